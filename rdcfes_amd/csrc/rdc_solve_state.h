// rdc_solve_state.h — what the cached artefacts of the linear solve are worth: the one rule by which the solve entries of the C-ABI
// (rdc_capi_solve.hip) clear and set the validity flags the observers read -- rdc_csr_matvec_f32 (f32_copy), rdc_solve_mg_level_download
// (mg_values), rdc_solve_ilu_download (ilu_factored), rdc_solve_gmres_stats (gmres_*).  Pure and host only, like rdc_path.h (no HIP, no
// allocation, no context; tests/host_solve_state_shim.cpp); no entry assigns a flag itself.  DESIGN.md 2 has the table this implements.
#ifndef RDC_SOLVE_STATE_H
#define RDC_SOLVE_STATE_H

#include "../../include/rdc_assembly.h"

namespace rdc {

struct SolveValid {
  bool f32_copy = false;      // val32 holds a usable fp32 copy (of the values at the time it was built)
  bool mg_values = false;     // mg_val and the D^-1 of the work buffer hold what the last cycle built, and nothing has run over them since
  bool ilu_factored = false;  // ilu_val holds the factor of the last ILU(0) hook or solve
  bool gmres_solved = false;  // a GMRES solve has run on this mesh: gmres_restart / gmres_cycles describe the last one
  int gmres_restart = 0, gmres_cycles = 0;
  bool gmres_dist = false;    // ... and it was a partitioned one (rdc_solve_dist_gmres): its basis slots have ghost tails
};

// rdc_csr_scale_f32 (a mixed call: it builds the copy) | rdc_solve, _mixed | rdc_solve_gmres_arnoldi | rdc_solve_mg_apply |
// rdc_solve_ilu_apply, _local_apply | rdc_solve_dist, _dist_mg, _dist_gmres | rdc_solve_dist_plan, _plan_peers (these two only enter).
// rdc_solve_dist_gmres_arnoldi is ARNOLDI with SolveCall::dist.
enum class SolveEntry { SCALE_F32, SOLVE, ARNOLDI, MG_APPLY, ILU_APPLY, DIST, DIST_PLAN };

struct SolveCall {
  SolveEntry entry;
  int precond = RDC_PRECOND_NONE;   // as the caller gave it
  bool mixed = false;               // the call rebuilds the fp32 copy from the current values
  bool gmres = false;               // the call needs the state of GMRES ("solve_method" = 1, rdc_solve_dist_gmres, the Arnoldi hooks)
  bool dist = false;                // the call is partitioned (entry DIST implies it; the collective Arnoldi hook sets it)
  bool partitioned() const { return dist || entry == SolveEntry::DIST; }
  bool ilu() const { return entry == SolveEntry::ILU_APPLY || precond == RDC_PRECOND_ILU0 || precond == RDC_PRECOND_ILU0_LOCAL; }
  bool multigrid() const { return entry == SolveEntry::MG_APPLY || precond == RDC_PRECOND_MULTIGRID || precond == RDC_PRECOND_MULTIGRID_GS_LOCAL; }
};

struct SolveOutcome {
  bool ran = false;           // the device work ran to its end (no HIP error)
  bool comm_failed = false;   // a callback of the communicator returned non-zero (partitioned solves)
  int bad_blocks = 0;         // diagonal blocks or pivots that are not invertible (the hooks, rdc_csr_scale_f32)
  int matrix_bits = 64;       // what a mixed call streamed: 64 = the copy overflowed fp32 and was given up
  int reason = RDC_SOLVE_CONVERGED;          // rdc_solve_info::reason (the solves)
  int gmres_restart = 0, gmres_cycles = 0;   // of a GMRES solve
};

// On entry, behind the mesh check and before the arguments are looked at: every call that runs or plans a solve rewrites D^-1 in the
// work buffer or lays the buffer out anew, so the values of a multigrid cycle are gone even if the call is then refused.
inline void solve_valid_enter(SolveValid& v, SolveEntry) { v.mg_values = false; }

// After the last refusal, before the first device view: what this call is about to rebuild is not valid while it does.
inline void solve_valid_begin(SolveValid& v, const SolveCall& call) {
  if (call.mixed) v.f32_copy = false;
  if (call.ilu()) v.ilu_factored = false;
}

// On leaving.  A call that did not run to its end, or lost its communicator, vouches for nothing it began to rebuild.  The hooks
// report bad blocks after this: the factor and the levels are there to be downloaded all the same, the fp32 copy is not.
inline void solve_valid_leave(SolveValid& v, const SolveCall& call, const SolveOutcome& o) {
  if (!o.ran || o.comm_failed) return;
  if (call.mixed) v.f32_copy = o.matrix_bits == 32 && o.bad_blocks == 0 && o.reason != RDC_SOLVE_BAD_DIAGONAL;
  if (call.ilu()) v.ilu_factored = true;
  v.mg_values = call.multigrid() && !call.partitioned();   // a partitioned hierarchy has ghost layers: no download
  if ((call.entry != SolveEntry::SOLVE && call.entry != SolveEntry::DIST) || !call.gmres) return;
  v.gmres_solved = true;
  v.gmres_dist = call.entry == SolveEntry::DIST;
  v.gmres_restart = o.gmres_restart;
  v.gmres_cycles = o.gmres_cycles;
}

}  // namespace rdc
#endif
