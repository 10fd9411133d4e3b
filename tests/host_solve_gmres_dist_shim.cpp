// CPU build of the layout of the GMRES state in its partitioned form (rdcfes_amd/csrc/rdc_solve.h, gmres_carve with n_nodes) for
// tests/test_host_solve_gmres_dist.py: basis slots with the stride of a ghosted vector, and the buffer of the wide all-reduce; and what the
// validity rule of rdc_solve_state.h makes of the two partitioned GMRES entries.
#include "../rdcfes_amd/csrc/rdc_solve.h"
#include "../rdcfes_amd/csrc/rdc_solve_state.h"

extern "C" {

// out[0 .. 12) = offsets in doubles of V, H, R, cs, sn, g, y, hpass, scal, red, partials, rec from the base (red: -1 if the form has
// none); out[12 .. 18) = bytes, basis_bytes, partial_count, vec_blocks, stride, n.  n_nodes < 0: the single-partition form.
void shim_gmres_carve_dist(int nvar, int64_t n_owned, int64_t n_nodes, int restart, int64_t* out) {
  double* base = (double*)(uintptr_t)4096;   // never dereferenced
  const rdc::GmresState g = rdc::gmres_carve(nvar, n_owned, restart, base, n_nodes);
  const double* part[12] = {g.V, g.H, g.R, g.cs, g.sn, g.g, g.y, g.hpass, g.scal, g.red, g.partials, (const double*)g.rec};
  for (int i = 0; i < 12; i++) out[i] = part[i] ? (int64_t)(part[i] - base) : -1;
  const rdc::GmresState measured = rdc::gmres_carve(nvar, n_owned, restart, nullptr, n_nodes);
  out[12] = (int64_t)measured.bytes; out[13] = (int64_t)g.basis_bytes; out[14] = g.partial_count; out[15] = g.vec_blocks; out[16] = g.stride;
  out[17] = g.n;
  if (measured.bytes != g.bytes || measured.V != nullptr || measured.red != nullptr || measured.rec != nullptr) out[12] = -1;
}

// The validity rule (rdc_solve_state.h) for a call that ran to its end with the multigrid preconditioner: entry, gmres and dist as the
// C-ABI sets them.  out = mg_values, gmres_solved, gmres_dist, gmres_restart, gmres_cycles, from a state that had mg_values and the
// record of a single-partition GMRES solve (restart 9, 1 cycle).
void shim_valid_after(int entry, int gmres, int dist, int restart, int cycles, int* out) {
  rdc::SolveValid v;
  v.mg_values = true; v.gmres_solved = true; v.gmres_restart = 9; v.gmres_cycles = 1;
  rdc::SolveCall call{(rdc::SolveEntry)entry, RDC_PRECOND_MULTIGRID, false, gmres != 0};
  call.dist = dist != 0;
  rdc::solve_valid_enter(v, call.entry);
  rdc::solve_valid_begin(v, call);
  rdc::SolveOutcome o;
  o.ran = true; o.gmres_restart = restart; o.gmres_cycles = cycles;
  rdc::solve_valid_leave(v, call, o);
  out[0] = v.mg_values; out[1] = v.gmres_solved; out[2] = v.gmres_dist; out[3] = v.gmres_restart; out[4] = v.gmres_cycles;
}

int shim_gmres_wide_max() { return rdc::GMRES_WIDE_MAX; }

}  // extern "C"
