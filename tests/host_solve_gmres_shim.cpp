// CPU build of the GMRES functions of rdcfes_amd/csrc/rdc_solve.h for tests/test_host_solve_gmres.py: the Givens step and the back
// substitution exactly as k_gmres_finalize and k_gmres_solve_y run them, and the layout of the state (gmres_carve).
#include "../rdcfes_amd/csrc/rdc_solve.h"

extern "C" {

// Least squares min || beta e_0 - H y || over the leading k columns of the raw Hessenberg matrix H (column-major, leading dimension
// m + 1): the Givens step column after column, then the back substitution.  R, cs, sn, g: caller's buffers of the sizes of
// gmres_carve ((m + 1) * m, m, m, m + 1).  flags[j] = what the step of column j returned; a column that is not taken ends the
// sweep.  Returns the columns taken; *y_ok = the back substitution over them was finite; *est = |g[taken]|.
int shim_gmres_lstsq(int m, int k, const double* H, double beta, double* R, double* cs, double* sn, double* g, double* y, int* flags,
                     int* y_ok, double* est) {
  const int ld = m + 1;
  g[0] = beta;
  int taken = 0;
  for (int j = 0; j < k; j++) {
    flags[j] = rdc::gmres_givens_step(j, H + (int64_t)j * ld, R + (int64_t)j * ld, cs, sn, g);
    if (flags[j]) break;
    taken++;
  }
  *y_ok = rdc::gmres_back_substitute(ld, taken, R, g, y) ? 1 : 0;
  *est = fabs(g[taken]);
  return taken;
}

// the layout: out[0 .. 11) = offsets in doubles of V, H, R, cs, sn, g, y, hpass, scal, partials, rec from the base (placed on a
// base of address 0 + 8); out[11 .. 16) = bytes, basis_bytes, partial_count, vec_blocks, stride
void shim_gmres_carve(int nvar, int64_t n_owned, int restart, int64_t* out) {
  double* base = (double*)(uintptr_t)4096;   // never dereferenced
  const rdc::GmresState g = rdc::gmres_carve(nvar, n_owned, restart, base);
  const double* part[11] = {g.V, g.H, g.R, g.cs, g.sn, g.g, g.y, g.hpass, g.scal, g.partials, (const double*)g.rec};
  for (int i = 0; i < 11; i++) out[i] = (int64_t)(part[i] - base);
  const rdc::GmresState measured = rdc::gmres_carve(nvar, n_owned, restart, nullptr);
  out[11] = (int64_t)measured.bytes; out[12] = (int64_t)g.basis_bytes; out[13] = g.partial_count; out[14] = g.vec_blocks; out[15] = g.stride;
  if (measured.bytes != g.bytes || measured.V != nullptr || measured.rec != nullptr) out[11] = -1;
}

int shim_gmres_constants(int which) {
  const int v[] = {rdc::GMRES_MAX_RESTART, rdc::GMRES_DEFAULT_RESTART, rdc::GMRES_NOT_FINITE, rdc::GMRES_HAPPY, rdc::GMRES_SINGULAR,
                   rdc::GMRES_SCALARS, (int)sizeof(rdc::GmresRec), rdc::VEC_PER_BLOCK};
  return v[which];
}

}  // extern "C"
