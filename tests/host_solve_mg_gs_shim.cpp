// g++ build of the colouring of the Gauss-Seidel smoother (rdcfes_amd/csrc/rdc_solve.h: mg_colour, mg_gs_place) for
// tests/test_host_solve_mg_gs.py: the colour lists of every level of a hierarchy and their placement, callable from ctypes.
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {
std::vector<rdc::MgColours> g_cols;

template <class T>
int64_t give(const std::vector<T>& v, void* out) {
  if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
  return (int64_t)v.size();
}
}  // namespace

extern "C" {

// builds the hierarchy below a matrix of n nodes and colours every level; returns the number of levels, -1 if mg_build refuses,
// -(2 + l) if mg_colour refuses level l
int shim_gs_colour(int64_t n, const int64_t* bptr, const int32_t* bcol) {
  std::vector<rdc::MgLevelHost> steps;
  if (!rdc::mg_build(n, bptr, bcol, steps)) return -1;
  g_cols.assign(steps.size() + 1, rdc::MgColours());
  for (size_t l = 0; l < g_cols.size(); l++) {
    const bool ok = l == 0 ? rdc::mg_colour(n, bptr, bcol, g_cols[0])
                           : rdc::mg_colour(steps[l - 1].n, steps[l - 1].bptr.data(), steps[l - 1].bcol.data(), g_cols[l]);
    if (!ok) return -(2 + (int)l);
  }
  return (int)g_cols.size();
}

// list `which` of level `level` (0 colour, 1 cptr, 2 nodes): copies it to `out` if given, returns its length
int64_t shim_gs_list(int level, int which, void* out) {
  if (level < 0 || level >= (int)g_cols.size()) return -1;
  const rdc::MgColours& C = g_cols[(size_t)level];
  switch (which) {
    case 0: return give(C.colour, out);
    case 1: return give(C.cptr, out);
    case 2: return give(C.nodes, out);
  }
  return -1;
}

// mg_colour on one pattern alone: 1 = proper, 0 = refused
int shim_gs_colour_one(int64_t n, const int64_t* bptr, const int32_t* bcol) {
  rdc::MgColours C;
  return rdc::mg_colour(n, bptr, bcol, C) ? 1 : 0;
}

// Places the lists of the last shim_gs_colour: measures, then places into `arena` (arena_bytes; null: measure only).  Returns the
// measured bytes, -1 if the arena is too small, -2 if the two passes disagree.  off[2 l], off[2 l + 1]: byte offsets of the node list
// and the pointer array of level l in the arena; what arrived there is for the caller to compare.
int64_t shim_gs_place(char* arena, int64_t arena_bytes, int64_t* off, int32_t* n_colours) {
  rdc::MgArena a;
  rdc::MgGsDev g;
  rdc::mg_gs_place(g_cols, a, g, [](void*, const void*, size_t) {});
  const int64_t bytes = (int64_t)a.used;
  if (!arena) return bytes;
  if (arena_bytes < bytes) return -1;
  a = rdc::MgArena{arena};
  rdc::mg_gs_place(g_cols, a, g, [](void* at, const void* list, size_t n) { std::memcpy(at, list, n); });
  if ((int64_t)a.used != bytes || g.n_levels != (int)g_cols.size()) return -2;
  for (int l = 0; l < g.n_levels; l++) {
    off[2 * l] = (const char*)g.lv[l].nodes - arena;
    off[2 * l + 1] = (const char*)g.lv[l].cptr - arena;
    n_colours[l] = g.lv[l].n_colours;
    if (g.lv[l].cptr_host != g_cols[(size_t)l].cptr.data()) return -2;
  }
  return bytes;
}

int shim_gs_constants(int* out) {
  out[0] = rdc::MG_GS_FUSED_NODES;
  out[1] = (int)rdc::MG_ALIGN;
  return 2;
}

}
