// g++ build of the multigrid-across-ranks part of rdcfes_amd/csrc/rdc_solve.h for tests/test_host_solve_mg_dist.py: the ranks of a
// world live side by side in this process, and the test drives every rank through the steps of a coarsening (mg_dist_aggregate,
// then mg_dist_coarsen on the aggregate numbers its numpy exchange delivers), as rdc_solve_dist_mg drives one rank between its
// two collective calls.
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {
struct RankState {
  std::vector<int64_t> bptr0;
  std::vector<int32_t> bcol0;
  std::vector<rdc::MgHalo> halos;        // halos[l]: the ghost layer of level l
  std::vector<rdc::MgLevelHost> steps;   // steps[l]: level l -> l + 1
  rdc::MgLevelHost pending;              // aggregated, not yet coarsened
};
std::vector<RankState> g_ranks;

template <class T>
int64_t give(const std::vector<T>& v, void* out) {
  if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
  return (int64_t)v.size();
}

RankState* rank_of(int r) { return r >= 0 && r < (int)g_ranks.size() ? &g_ranks[(size_t)r] : nullptr; }
}  // namespace

extern "C" {

void shim_dist_world(int world) { g_ranks.assign((size_t)world, RankState()); }

// level 0 of a rank: its pattern (owned rows over local nodes) and its plan with the per-peer counts; returns mg_halo_plan's code
int shim_dist_plan(int r, int64_t n_owned, int64_t n_ghost, const int64_t* bptr, const int32_t* bcol, int64_t n_send,
                   const int32_t* send_nodes, int n_peers, const int64_t* send_count, const int64_t* ghost_count) {
  RankState* S = rank_of(r);
  if (!S) return -1;
  *S = RankState();
  S->bptr0.assign(bptr, bptr + n_owned + 1);
  S->bcol0.assign(bcol, bcol + bptr[n_owned]);
  S->halos.resize(1);
  return rdc::mg_halo_plan(n_owned, n_ghost, n_send, send_nodes, n_peers, send_count, ghost_count, S->halos[0]);
}

// step 1 on the rank's last level: ids_out [its send entries] = what the exchange sends; returns the number of aggregates
int64_t shim_dist_aggregate(int r, double* ids_out) {
  RankState* S = rank_of(r);
  if (!S || S->halos.empty()) return -1;
  const bool top = S->steps.empty();
  rdc::mg_dist_aggregate(S->halos.back(), top ? S->bptr0.data() : S->steps.back().bptr.data(),
                         top ? S->bcol0.data() : S->steps.back().bcol.data(), S->pending, ids_out);
  return S->pending.n;
}

// step 2: ids_in [ghosts of the last level] as delivered; 1 = the level was added, 0 = refused
int shim_dist_coarsen(int r, const double* ids_in) {
  RankState* S = rank_of(r);
  if (!S || S->halos.empty()) return -1;
  const bool top = S->steps.empty();
  rdc::MgHalo C;
  // the fine pattern must outlive the move below: take its pointers first, they point into vectors that do not reallocate
  const int64_t* bptr = top ? S->bptr0.data() : S->steps.back().bptr.data();
  const int32_t* bcol = top ? S->bcol0.data() : S->steps.back().bcol.data();
  if (!rdc::mg_dist_coarsen(S->halos.back(), bptr, bcol, ids_in, S->pending, C)) return 0;
  S->steps.reserve(rdc::MG_MAX_LEVELS);
  S->steps.push_back(std::move(S->pending));
  S->halos.push_back(std::move(C));
  return 1;
}

int shim_dist_goes_on(int levels, double nodes, double merged) { return rdc::mg_dist_goes_on(levels, nodes, merged) ? 1 : 0; }

// list `which` of rank r.  0 .. 7: of step `level` as shim_mg_list of host_solve_mg_shim.cpp (0 agg, 1 mptr, 2 member, 3 bptr, 4 bcol,
// 5 cptr, 6 cidx, 7 cnode); 10 .. 14: of the ghost layer of level `level` (10 send_off, 11 ghost_off, 12 send_nodes, 13 send_ptr,
// 14 send_slot); 100 / 101 / 102: n_fine, n, n_pass1 of the step; 110 / 111: n_owned, n_ghost of the layer; 120: levels of the rank
int64_t shim_dist_list(int r, int level, int which, void* out) {
  RankState* S = rank_of(r);
  if (!S) return -1;
  if (which == 120) return (int64_t)S->halos.size();
  if ((which >= 10 && which < 100) || which >= 110) {
    if (level < 0 || level >= (int)S->halos.size()) return -1;
    const rdc::MgHalo& H = S->halos[(size_t)level];
    switch (which) {
      case 10: return give(H.send_off, out);
      case 11: return give(H.ghost_off, out);
      case 12: return give(H.send_nodes, out);
      case 13: return give(H.send_ptr, out);
      case 14: return give(H.send_slot, out);
      case 110: return H.n_owned;
      case 111: return H.n_ghost;
    }
    return -1;
  }
  if (level < 0 || level >= (int)S->steps.size()) return -1;
  const rdc::MgLevelHost& L = S->steps[(size_t)level];
  switch (which) {
    case 0: return give(L.agg, out);
    case 1: return give(L.mptr, out);
    case 2: return give(L.member, out);
    case 3: return give(L.bptr, out);
    case 4: return give(L.bcol, out);
    case 5: return give(L.cptr, out);
    case 6: return give(L.cidx, out);
    case 7: return give(L.cnode, out);
    case 100: return L.n_fine;
    case 101: return L.n;
    case 102: return L.n_pass1;
  }
  return -1;
}

// bytes of the two device arenas of rank r for nvar unknowns per node (mg_place measuring, with the ghost layers): idx, val
int shim_dist_bytes(int r, int nvar, int64_t* out) {
  RankState* S = rank_of(r);
  if (!S || S->halos.empty()) return -1;
  rdc::MgArena idx, val;
  rdc::MgDev g;
  rdc::mg_place(S->steps, nvar, S->halos[0].n_owned, S->bptr0.back(), idx, val, g, [](void*, const void*, size_t) {}, &S->halos);
  out[0] = (int64_t)idx.used; out[1] = (int64_t)val.used;
  return g.n_levels;
}

}
