// Stand-alone run of the multigrid-across-ranks host code of rdcfes_amd/csrc/rdc_solve.h for tools/asan_solve_mg_dist.sh: no device,
// no Python.  Worlds: a 7-point grid graph cut into 2 and 3 slabs, a 5-point one with a rank whose nodes are mutually unconnected,
// and a single rank.  Every rank goes through mg_dist_aggregate / mg_dist_coarsen with an in-process exchange of the aggregate
// numbers; returns 0 if on every level the two sides of every pair name the same aggregates in the same order and, for 3 and 5
// unknowns per node, the device layout of mg_place with its ghost layers fits what it measured: host buffers of exactly the measured
// sizes stand in for the two arenas, every list is copied into its slot and every other array is filled, so the sanitizer sees each write.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {

struct Rank {
  std::vector<int64_t> bptr;   // owned rows over local nodes
  std::vector<int32_t> bcol;
  std::vector<int> peers;      // rank ids, ascending
  std::vector<rdc::MgHalo> halos;
  std::vector<rdc::MgLevelHost> steps;
};

// ranks of a global graph (adjacency without the diagonal) with owner[node]: owned nodes first in ascending global id, ghosts behind
// them grouped by owner, ascending; the send list for q = the owned nodes q sees, ascending (the order of q's ghosts from here)
std::vector<Rank> split(const std::vector<std::vector<int32_t>>& adj, const std::vector<int>& owner, int world) {
  std::vector<Rank> out((size_t)world);
  const int32_t n = (int32_t)adj.size();
  for (int r = 0; r < world; r++) {
    std::map<int32_t, int32_t> local;
    std::vector<int32_t> owned;
    std::vector<std::vector<int32_t>> ghosts((size_t)world), sends((size_t)world);
    for (int32_t i = 0; i < n; i++)
      if (owner[(size_t)i] == r) owned.push_back(i);
    for (int32_t i : owned) {
      for (int32_t j : adj[(size_t)i])
        if (owner[(size_t)j] != r) { ghosts[(size_t)owner[(size_t)j]].push_back(j); sends[(size_t)owner[(size_t)j]].push_back(i); }
    }
    for (int32_t i : owned) { const int32_t at = (int32_t)local.size(); local[i] = at; }
    std::vector<int64_t> sc, gc;
    std::vector<int32_t> send_nodes;
    for (int q = 0; q < world; q++) {
      auto uniq = [](std::vector<int32_t>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
      uniq(ghosts[(size_t)q]); uniq(sends[(size_t)q]);
      if (ghosts[(size_t)q].empty() && sends[(size_t)q].empty()) continue;
      out[(size_t)r].peers.push_back(q);
      for (int32_t g : ghosts[(size_t)q]) { const int32_t at = (int32_t)local.size(); local[g] = at; }
      for (int32_t s : sends[(size_t)q]) send_nodes.push_back(local[s]);
      sc.push_back((int64_t)sends[(size_t)q].size()); gc.push_back((int64_t)ghosts[(size_t)q].size());
    }
    Rank& R = out[(size_t)r];
    R.bptr.push_back(0);
    for (int32_t i : owned) {
      std::vector<int32_t> row{local[i]};
      for (int32_t j : adj[(size_t)i]) row.push_back(local[j]);
      std::sort(row.begin(), row.end());
      R.bcol.insert(R.bcol.end(), row.begin(), row.end());
      R.bptr.push_back((int64_t)R.bcol.size());
    }
    R.halos.resize(1);
    if (rdc::mg_halo_plan((int64_t)owned.size(), (int64_t)local.size() - (int64_t)owned.size(), (int64_t)send_nodes.size(), send_nodes.data(),
                          (int)sc.size(), sc.data(), gc.data(), R.halos[0]))
      std::exit(90);
  }
  return out;
}

// the collective build, all ranks in step; 0, or 1: refused, 2: ranks disagree on a segment length
int build(std::vector<Rank>& W) {
  for (;;) {
    std::vector<std::vector<double>> sent(W.size());
    std::vector<rdc::MgLevelHost> L(W.size());
    double nodes = 0.0, merged = 0.0;
    for (size_t r = 0; r < W.size(); r++) {
      const rdc::MgHalo& F = W[r].halos.back();
      sent[r].assign((size_t)F.n_send(), -1.0);   // exactly the send entries: a write past them is caught
      rdc::mg_dist_aggregate(F, W[r].steps.empty() ? W[r].bptr.data() : W[r].steps.back().bptr.data(),
                             W[r].steps.empty() ? W[r].bcol.data() : W[r].steps.back().bcol.data(), L[r], sent[r].data());
      nodes += (double)F.n_owned; merged += L[r].n < F.n_owned ? 1.0 : 0.0;
    }
    if (!rdc::mg_dist_goes_on((int)W[0].halos.size(), nodes, merged)) return 0;
    for (size_t r = 0; r < W.size(); r++) {
      const rdc::MgHalo& F = W[r].halos.back();
      std::vector<double> got((size_t)F.n_ghost, -1.0);
      for (size_t k = 0; k < W[r].peers.size(); k++) {
        const Rank& Q = W[(size_t)W[r].peers[k]];
        const size_t j = (size_t)(std::find(Q.peers.begin(), Q.peers.end(), (int)r) - Q.peers.begin());
        const rdc::MgHalo& FQ = Q.halos[W[r].halos.size() - 1];
        if (j >= Q.peers.size() || FQ.send_off[j + 1] - FQ.send_off[j] != F.ghost_off[k + 1] - F.ghost_off[k]) return 2;
        std::copy(sent[(size_t)W[r].peers[k]].begin() + FQ.send_off[j], sent[(size_t)W[r].peers[k]].begin() + FQ.send_off[j + 1],
                  got.begin() + F.ghost_off[k]);
      }
      rdc::MgHalo C;
      if (!rdc::mg_dist_coarsen(F, W[r].steps.empty() ? W[r].bptr.data() : W[r].steps.back().bptr.data(),
                                W[r].steps.empty() ? W[r].bcol.data() : W[r].steps.back().bcol.data(), got.data(), L[r], C))
        return 1;
      W[r].steps.reserve(rdc::MG_MAX_LEVELS);
      W[r].steps.push_back(std::move(L[r]));
      W[r].halos.push_back(std::move(C));   // (the peers look at the level above: halos of this level are complete only behind the loop)
    }
  }
}

// 15: the passes disagree; 16: not aligned; 17: leaves its arena; 18: overlap, or a list did not arrive
int check_layout(const Rank& R, int nv) {
  const int64_t n0 = R.halos[0].n_owned, blocks = R.bptr.back();
  rdc::MgArena idx, val;
  rdc::MgDev g;
  rdc::mg_place(R.steps, nv, n0, blocks, idx, val, g, [](void*, const void*, size_t) {}, &R.halos);
  const size_t ibytes = idx.used, vbytes = val.used;
  if (g.ph || g.sh || g.t0 || ibytes % rdc::MG_ALIGN || vbytes % rdc::MG_ALIGN || vbytes == 0) return 15;
  char* ibuf = ibytes ? (char*)std::aligned_alloc(rdc::MG_ALIGN, ibytes) : nullptr;
  char* vbuf = (char*)std::aligned_alloc(rdc::MG_ALIGN, vbytes);
  idx = rdc::MgArena{ibuf};
  val = rdc::MgArena{vbuf};
  rdc::mg_place(R.steps, nv, n0, blocks, idx, val, g, [](void* at, const void* list, size_t bytes) { std::memcpy(at, list, bytes); }, &R.halos);
  struct Span { const char* at; size_t bytes; };
  std::vector<Span> in_idx, in_val;
  auto lst = [&](const auto* at, const auto& v) { in_idx.push_back({(const char*)at, v.size() * sizeof(v[0])}); };
  auto vec = [&](double* at, int64_t doubles) {
    in_val.push_back({(const char*)at, (size_t)doubles * sizeof(double)});
    if (at) std::memset(at, 0x5a, (size_t)doubles * sizeof(double));
  };
  int rc = idx.used != ibytes || val.used != vbytes || g.n_levels != (int)R.steps.size() + 1 ? 15 : 0;
  const int64_t nn = std::max<int64_t>(n0 * nv, 1), ng = std::max<int64_t>((n0 + R.halos[0].n_ghost) * nv, 1);
  vec(g.ph, ng); vec(g.sh, ng); vec(g.t0, nn);
  for (size_t l = 0; l < R.steps.size() && !rc; l++) {
    const rdc::MgLevelHost& L = R.steps[l];
    const rdc::MgHalo& H = R.halos[l + 1];
    const rdc::MgLevelDev& D = g.lv[l + 1];
    if (D.n != L.n || D.blocks != (int64_t)L.bcol.size() || D.n_ghost != H.n_ghost || D.n_send != H.n_send()) rc = 15;
    if ((int64_t)L.agg.size() != L.n_fine + R.halos[l].n_ghost) rc = 15;
    lst(D.agg, L.agg); lst(D.mptr, L.mptr); lst(D.member, L.member); lst(D.bptr, L.bptr); lst(D.bcol, L.bcol); lst(D.brow, L.brow);
    lst(D.cptr, L.cptr); lst(D.cidx, L.cidx); lst(D.cnode, L.cnode); lst(D.send_ptr, H.send_ptr); lst(D.send_slot, H.send_slot);
    vec(D.val, D.blocks * nv * nv); vec(D.dinv, D.n * nv * nv); vec(D.x, (D.n + D.n_ghost) * nv); vec(D.r, D.n * nv); vec(D.t, D.n * nv);
    vec(D.send, std::max<int64_t>(D.n_send * nv, 1));
    for (int32_t c : L.bcol)
      if (c < 0 || c >= L.n + H.n_ghost) rc = 17;      // every column is an owned aggregate or a coarse ghost: x covers it
    for (int32_t s : H.send_slot)
      if (s < 0 || s >= H.n_send()) rc = 17;
  }
  auto spans = [](std::vector<Span>& a, const char* base, size_t bytes) {
    a.erase(std::remove_if(a.begin(), a.end(), [](const Span& s) { return !s.bytes; }), a.end());   // an empty list takes no room
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
  for (size_t l = 0; l < R.steps.size() && !rc; l++)
    if (std::memcmp(g.lv[l + 1].send_ptr, R.halos[l + 1].send_ptr.data(), R.halos[l + 1].send_ptr.size() * 8) ||
        std::memcmp(g.lv[l + 1].agg, R.steps[l].agg.data(), R.steps[l].agg.size() * 4))
      rc = 18;
  std::free(ibuf);
  std::free(vbuf);
  return rc;
}

int check(const char* name, const std::vector<std::vector<int32_t>>& adj, const std::vector<int>& owner, int world) {
  std::vector<Rank> W = split(adj, owner, world);
  if (int rc = build(W)) return rc;
  std::printf("%s, %d ranks:", name, world);
  for (size_t l = 0; l < W[0].halos.size(); l++) {
    int64_t n = 0;
    for (const Rank& R : W) n += R.halos[l].n_owned;
    std::printf(" %s%lld", l ? "-> " : "", (long long)n);
  }
  std::printf("\n");
  for (size_t r = 0; r < W.size(); r++) {
    if (W[r].halos.size() != W[0].halos.size()) return 3;
    for (size_t l = 1; l < W[r].halos.size(); l++)
      for (size_t k = 0; k < W[r].peers.size(); k++) {   // the coarse send segment for q has the length of q's coarse ghost segment from here
        const Rank& Q = W[(size_t)W[r].peers[k]];
        const size_t j = (size_t)(std::find(Q.peers.begin(), Q.peers.end(), (int)r) - Q.peers.begin());
        if (W[r].halos[l].send_off[k + 1] - W[r].halos[l].send_off[k] != Q.halos[l].ghost_off[j + 1] - Q.halos[l].ghost_off[j]) return 4;
      }
    for (int nv : {3, 5})
      if (int rc = check_layout(W[r], nv)) return rc;
  }
  return 0;
}

std::vector<std::vector<int32_t>> grid(int nx, int ny, int nz) {
  std::vector<std::vector<int32_t>> adj((size_t)nx * ny * nz);
  auto id = [=](int i, int j, int k) { return (int32_t)((i * ny + j) * nz + k); };
  auto link = [&](int32_t a, int32_t b) { adj[(size_t)a].push_back(b); adj[(size_t)b].push_back(a); };
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++)
      for (int k = 0; k < nz; k++) {
        if (i + 1 < nx) link(id(i, j, k), id(i + 1, j, k));
        if (j + 1 < ny) link(id(i, j, k), id(i, j + 1, k));
        if (k + 1 < nz) link(id(i, j, k), id(i, j, k + 1));
      }
  return adj;
}

}  // namespace

int main() {
  int rc;
  const auto g = grid(9, 8, 8);
  for (int world : {1, 2, 3}) {
    std::vector<int> owner(g.size());
    for (size_t i = 0; i < g.size(); i++) owner[i] = (int)(i / 64) * world / 9;   // slabs of whole i-planes
    if ((rc = check("grid 9 x 8 x 8", g, owner, world))) return 20 * world + rc;
  }
  auto u = grid(5, 10, 1);      // rank 1: ten nodes coupled to one node of rank 0 each and to nothing else
  std::vector<int> owner(60, 0);
  for (int i = 0; i < 10; i++) { u.push_back({(int32_t)i}); u[(size_t)i].push_back(50 + i); owner[(size_t)(50 + i)] = 1; }
  if ((rc = check("grid 5 x 10 and 10 unconnected nodes", u, owner, 2))) return 80 + rc;
  return 0;
}
