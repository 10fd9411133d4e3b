// g++ build of the multigrid part of rdcfes_amd/csrc/rdc_solve.h for tests/test_host_solve_mg.py: aggregation, coarse
// pattern and contribution lists of a whole hierarchy, and the level-1 Galerkin summand, callable from ctypes.
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {
std::vector<rdc::MgLevelHost> g_steps;

template <class T>
int64_t give(const std::vector<T>& v, void* out) {
  if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
  return (int64_t)v.size();
}
}  // namespace

extern "C" {

// builds the hierarchy below a matrix of n nodes; returns the number of coarsening steps, -1 if mg_build refuses
int shim_mg_build(int64_t n, const int64_t* bptr, const int32_t* bcol) {
  return rdc::mg_build(n, bptr, bcol, g_steps) ? (int)g_steps.size() : -1;
}

// list `which` of step `step` (0 agg, 1 mptr, 2 member, 3 bptr, 4 bcol, 5 cptr, 6 cidx, 7 cnode): copies it to `out` if given,
// returns its length; 100 / 101 / 102: n_fine, n, n_pass1
int64_t shim_mg_list(int step, int which, void* out) {
  if (step < 0 || step >= (int)g_steps.size()) return -1;
  const rdc::MgLevelHost& L = g_steps[(size_t)step];
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

int shim_mg_constants(int* out) {
  const int c[6] = {rdc::MG_AGG_CAP, rdc::MG_MIN_FREE, rdc::MG_COARSEST_NODES, rdc::MG_MAX_LEVELS, rdc::MG_COARSEST_SWEEPS,
                    rdc::MG_OMEGA_PERMILLE};
  std::memcpy(out, c, sizeof(c));
  return 6;
}

// out = dinv * a (nv x nv, row-major) as the Galerkin kernel forms the summands of level 1
int shim_scaled_block(int nv, const double* dinv, const double* a, double* out) {
  if (nv == 3) rdc::scaled_block<3>(*reinterpret_cast<const double (*)[3][3]>(dinv), *reinterpret_cast<const double (*)[3][3]>(a),
                                    *reinterpret_cast<double (*)[3][3]>(out));
  else if (nv == 5) rdc::scaled_block<5>(*reinterpret_cast<const double (*)[5][5]>(dinv), *reinterpret_cast<const double (*)[5][5]>(a),
                                         *reinterpret_cast<double (*)[5][5]>(out));
  else return -1;
  return 0;
}

}
