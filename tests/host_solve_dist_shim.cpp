// g++ build of rdcfes_amd/csrc/rdc_solve.h for tests/test_host_solve_dist.py: the plan check of a partitioned solve and the
// layout of the work buffer (carve), callable from ctypes.
#include "../rdcfes_amd/csrc/rdc_solve.h"

extern "C" {

// rdc::dist_plan_check; *where as there
int shim_plan_check(int64_t n_owned, const int64_t* bptr, const int32_t* bcol, int64_t n_int, int64_t n_send, const int32_t* send_nodes,
                    int64_t* where) {
  return rdc::dist_plan_check(n_owned, bptr, bcol, n_int, n_send, send_nodes, where);
}

// bytes of the work buffer: of rdc_solve (dist == 0), or of rdc_solve_dist with the given dimensions
int64_t shim_work_bytes(int nvar, int64_t n_owned, int dist, int64_t n_nodes, int64_t n_int, int64_t n_send) {
  const rdc::DistDims dd{n_nodes, n_int, n_send};
  return (int64_t)rdc::carve(nvar, n_owned, nullptr, dist ? &dd : nullptr).bytes;
}

// The arrays carve places, as (byte offset from the base, bytes) pairs in out[2 * i], out[2 * i + 1]; returns their number.
// Order: r, rh, p, v, s, t, dinv, partials, [send, rec,] scal.  *partials_needed = doubles the largest set of partials takes.
int shim_work_layout(int nvar, int64_t n_owned, int dist, int64_t n_nodes, int64_t n_int, int64_t n_send, int64_t* out,
                     int64_t* partials_needed) {
  const rdc::DistDims dd{n_nodes, n_int, n_send};
  alignas(16) static char origin[16];
  double* base = reinterpret_cast<double*>(origin);   // only differences of the pointers are taken
  const rdc::Work w = rdc::carve(nvar, n_owned, base, dist ? &dd : nullptr);
  const int64_t n = n_owned * nvar, ng = dist ? n_nodes * nvar : n;
  const int64_t parts = 2 * rdc::op_parts(n_owned, dist ? n_int : 0, rdc::SCALED);
  const int64_t parts32 = 2 * rdc::op_parts(n_owned, dist ? n_int : 0, rdc::F32);
  int64_t need = parts > parts32 ? parts : parts32;
  if (4 * w.node_blocks > need) need = 4 * w.node_blocks;
  if (3 * w.vec_blocks > need) need = 3 * w.vec_blocks;
  *partials_needed = need;
  const double* ptr[11] = {w.r, w.rh, w.p, w.v, w.s, w.t, w.dinv, w.partials, w.send, w.rec, (const double*)w.scal};
  const int64_t len[11] = {n, n, ng, n, ng, n, n * nvar, -1, n_send * nvar, rdc::DIST_RECORD, (int64_t)(sizeof(rdc::SolveScal) / sizeof(double))};
  int k = 0;
  for (int i = 0; i < 11; i++) {
    if (!ptr[i]) continue;
    out[2 * k] = (int64_t)((const char*)ptr[i] - (const char*)base);
    out[2 * k + 1] = len[i] * (int64_t)sizeof(double);
    k++;
  }
  return k;
}

}
