// rdc_newton.h — the device-resident Newton solve of the solid system (rdc_solid_newton, include/rdc_assembly.h): every decision
// of the loop and the layout of its work memory, as host functions that g++ compiles without a device (tests/host_newton_main.cpp).
// rdc_newton.hip only executes what newton_next hands out.
//
// The loop is SolidSystem::solve() of the host mirror (rdcfes_amd/host/rdc_host.h), which stands for libMesh's NewtonSolver:
//   assemble R, J | ||R|| against the two residual tolerances, the iteration count against the cap | J delta = -R from 0 |
//   u = u0 + step delta, step = 1, halved under "require_reduction" while ||R(u)|| is not below ||R(u0)|| and step >= 1e-3 |
//   ||step delta|| <= relative_step_tolerance ||u||: one residual-only assembly, converged by step.
// Two outcomes the mirror leaves open: RDC_SOLVE_MAX_ITS of the linear solve is used as it is; any other failure of it, and a
// residual norm that is not finite outside a reduction trial, end the call (LINEAR_FAILED, NOT_FINITE) with the coordinates of
// the saved iterate.  Inside a reduction trial a norm that is not finite is "not below": the step is halved, as the mirror does.
//
// Host traffic.  No matrix, rhs or vector crosses the bus between entry and exit.  Per Newton iteration the host reads the records
// rdc_solve reads, and one 64-byte record (NewtonRec: three sums) behind the full assembly and one behind every step or trial:
// ||R||^2 behind the assembly; ||step delta||^2, ||u||^2 and, where the step is tried, ||R(u)||^2 behind the step.
//
// Across ranks (rdc_solid_newton_dist).  The decisions are the same newton_next, fed global norms: every sum runs over the rows a
// rank owns and the whole record crosses the ranks in one allreduce_sum of NEWTON_REC_DOUBLES doubles before each host read.
// newton_linear_dispatch names the partitioned linear entry and the callbacks it needs; newton_carve_dist is the work memory with
// a ghost tail behind delta (the partitioned entries fill it with the owners' values) and the send buffer of the entry exchange.
#ifndef RDC_NEWTON_H
#define RDC_NEWTON_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rdc_assembly.h"

namespace rdc {

// ---- work memory: one allocation of the buffer group of the linear solve (buf.solve.newton), made at the first call on a mesh
constexpr int NEWTON_CHUNK = 1024;       // entries of a vector one workgroup of 256 sums: fixes the order of every sum
constexpr int NEWTON_ALIGN = 32;         // doubles: every part starts on a 256-byte boundary
constexpr int NEWTON_REC_DOUBLES = 8;    // the record the host reads: 64 bytes
enum { NEWTON_SUM_RESIDUAL = 0, NEWTON_SUM_STEP = 1, NEWTON_SUM_SOLUTION = 2 };   // NewtonRec::sum

struct NewtonRec { double sum[3]; double pad[NEWTON_REC_DOUBLES - 3]; };
static_assert(sizeof(NewtonRec) == 64, "the record of the Newton loop is 64 bytes");

// offsets in doubles from the start of the allocation; n = 3 * n_node entries of the coordinate array, which is the dof layout
struct NewtonWork {
  int64_t n = 0, n_owned = 0;      // entries of u0 (and of the coordinates); of delta and the rhs
  int64_t blocks = 0;              // workgroups of a pass over n entries: partials holds 2 per workgroup (k_newton_step)
  int64_t u0 = 0, delta = 0, partials = 0, rec = 0;
  size_t bytes = 0;
  int64_t n_delta = 0;             // entries of delta: n_owned, or n behind newton_carve_dist (a ghost tail the linear solve fills)
  int64_t send = 0, n_send = 0;    // newton_carve_dist: the packed coordinates of the plan's send nodes (3 per node); else empty
};

// the one statement of the layout; it only measures (nothing is dereferenced)
inline NewtonWork newton_carve(int64_t n_node, int64_t n_owned) {
  NewtonWork w;
  auto up = [](int64_t v) { return (v + NEWTON_ALIGN - 1) / NEWTON_ALIGN * NEWTON_ALIGN; };
  w.n = 3 * n_node;
  w.n_owned = 3 * n_owned;
  w.blocks = (w.n + NEWTON_CHUNK - 1) / NEWTON_CHUNK;
  int64_t at = 0;
  w.u0 = at; at += up(w.n);
  w.delta = at; at += up(w.n_owned);
  w.partials = at; at += up(2 * w.blocks);
  w.rec = at; at += NEWTON_REC_DOUBLES;
  w.bytes = (size_t)at * sizeof(double);
  w.n_delta = w.n_owned;
  w.send = w.rec;   // empty
  return w;
}

// The layout of rdc_solid_newton_dist: delta has all n entries (owned rows, then the ghost tail), and the send buffer of the one
// exchange the entry makes itself lies before the record.  Without ghosts and with an empty send list every offset and the size
// are those of newton_carve.
inline NewtonWork newton_carve_dist(int64_t n_node, int64_t n_owned, int64_t n_send_nodes) {
  NewtonWork w;
  auto up = [](int64_t v) { return (v + NEWTON_ALIGN - 1) / NEWTON_ALIGN * NEWTON_ALIGN; };
  w.n = 3 * n_node;
  w.n_owned = 3 * n_owned;
  w.n_delta = w.n;
  w.n_send = 3 * n_send_nodes;
  w.blocks = (w.n + NEWTON_CHUNK - 1) / NEWTON_CHUNK;
  int64_t at = 0;
  w.u0 = at; at += up(w.n);
  w.delta = at; at += up(w.n_delta);
  w.partials = at; at += up(2 * w.blocks);
  w.send = at; at += up(w.n_send);
  w.rec = at; at += NEWTON_REC_DOUBLES;
  w.bytes = (size_t)at * sizeof(double);
  return w;
}

// ---- the linear solve of rdc_solid_newton_dist: which partitioned entry runs, and which callbacks of rdc_solve_comm_wide must
// not be NULL for it.  exchange_begin, exchange_end and allreduce_sum always are (the loop itself uses them).
enum NewtonLinearEntry : int32_t { NEWTON_LINEAR_DIST = 0, NEWTON_LINEAR_DIST_MG = 1, NEWTON_LINEAR_DIST_GMRES = 2 };
enum { NEWTON_NEEDS_SIZED = 1, NEWTON_NEEDS_WIDE = 2 };
struct NewtonDispatch { NewtonLinearEntry entry; int32_t needs; };

inline NewtonDispatch newton_linear_dispatch(int32_t precond, int32_t solve_method) {
  const bool mg = precond == RDC_PRECOND_MULTIGRID || precond == RDC_PRECOND_MULTIGRID_GS_LOCAL;
  NewtonDispatch d;
  d.entry = solve_method == 1 ? NEWTON_LINEAR_DIST_GMRES : mg ? NEWTON_LINEAR_DIST_MG : NEWTON_LINEAR_DIST;
  d.needs = (mg ? NEWTON_NEEDS_SIZED : 0) | (solve_method == 1 ? NEWTON_NEEDS_WIDE : 0);
  return d;
}

inline bool newton_comm_complete(const rdc_solve_comm_wide& c, const NewtonDispatch& d) {
  const rdc_solve_comm& b = c.sized.base;
  if (!b.exchange_begin || !b.exchange_end || !b.allreduce_sum) return false;
  if ((d.needs & NEWTON_NEEDS_SIZED) && (!c.sized.exchange_sized_begin || !c.sized.exchange_sized_end)) return false;
  if ((d.needs & NEWTON_NEEDS_WIDE) && !c.allreduce_sum_wide) return false;
  return true;
}

// ---- what the entry refuses of its parameters: null if they are fine, the message otherwise
inline const char* newton_check_params(const rdc_solid_newton_params& p) {
  if (p.max_nonlinear_iterations < 1 || p.max_nonlinear_iterations > 1000) return "max_nonlinear_iterations must be 1 .. 1000";
  if ((p.require_reduction != 0 && p.require_reduction != 1) || (p.mixed != 0 && p.mixed != 1)) return "require_reduction and mixed are 0 or 1";
  const double t[5] = {p.relative_step_tolerance, p.relative_residual_tolerance, p.absolute_residual_tolerance, p.linear.rel_tol, p.linear.abs_tol};
  for (double v : t)
    if (!(v >= 0.0) || !std::isfinite(v)) return "tolerances must be finite and not negative";
  if (p.linear.max_its < 1) return "linear.max_its must be at least 1";
  if (p.linear.precond < RDC_PRECOND_NONE || p.linear.precond > RDC_PRECOND_MULTIGRID_GS_LOCAL) return "unknown preconditioner";
  return nullptr;
}

// ---- the decisions
enum NewtonAction : int32_t {
  NEWTON_ASSEMBLE_FULL = 0,   // rdc_solid_assemble with the tangent, then ||R||                       -> norms.residual
  NEWTON_SOLVE = 1,           // u0 = coordinates, delta = 0, the linear solve                          -> norms.linear_*
  NEWTON_TRY_STEP = 2,        // coordinates = u0 + step delta -> norms.step_norm, solution_norm; where state.measure is set,
  NEWTON_HALVE = 3,           // ... a residual-only assembly there -> norms.residual.  HALVE: the same with the halved step
  NEWTON_ACCEPT = 4,          // the iteration is done; where state.measure is set, a residual-only assembly -> norms.residual
  NEWTON_FINISH = 5,          // state.info.reason is set; where state.restore is set, coordinates = u0 first (a step of length 0)
};

struct NewtonNorms {          // what the action just executed measured; the other fields are not read
  double residual = 0.0, step_norm = 0.0, solution_norm = 0.0;
  int32_t linear_reason = 0, linear_iterations = 0;
};

struct NewtonState {
  int32_t last = -1;          // the action handed out last (-1: none yet)
  int32_t it = 0;             // Newton iterations completed
  int32_t measure = 0, restore = 0;
  int32_t saved = 0;          // u0 holds an iterate whose residual was finite
  int32_t lin_its = 0, lin_reason = 0;   // of the solve of the iteration at hand
  double step = 1.0;
  double rn = 0.0;            // ||R(u0)|| of the iteration at hand
  rdc_solid_newton_info info = rdc_solid_newton_info();
};

inline NewtonAction newton_finish(NewtonState& s, int32_t reason, bool restore) {
  s.info.reason = reason;
  s.restore = restore ? 1 : 0;
  s.measure = 0;
  return NEWTON_FINISH;
}

// Every decision of the loop: from the state and what the last action measured to the next action.  Bounded: at most
// max_nonlinear_iterations iterations, each with at most 10 halvings (1 / 1024 < 1e-3).
inline NewtonAction newton_next(const rdc_solid_newton_params& p, NewtonState& s, const NewtonNorms& m) {
  rdc_solid_newton_info& I = s.info;
  NewtonAction a = NEWTON_FINISH;
  switch (s.last) {
    case -1:
      a = NEWTON_ASSEMBLE_FULL;
      break;
    case NEWTON_ASSEMBLE_FULL:
      I.assemblies++;
      if (s.it == 0) I.first_residual = m.residual;
      I.last_residual = m.residual;
      s.rn = m.residual;
      if (!std::isfinite(m.residual)) a = newton_finish(s, RDC_NEWTON_NOT_FINITE, s.saved != 0);
      else if (m.residual <= p.absolute_residual_tolerance || m.residual <= p.relative_residual_tolerance * I.first_residual)
        a = newton_finish(s, RDC_NEWTON_CONVERGED_RESIDUAL, false);
      else if (s.it >= p.max_nonlinear_iterations) a = newton_finish(s, RDC_NEWTON_MAX_ITS, false);
      else a = NEWTON_SOLVE;
      break;
    case NEWTON_SOLVE:
      s.saved = 1;
      s.lin_its = m.linear_iterations;
      s.lin_reason = m.linear_reason;
      I.linear_iterations += m.linear_iterations;
      I.last_linear_reason = m.linear_reason;
      if (m.linear_reason != RDC_SOLVE_CONVERGED && m.linear_reason != RDC_SOLVE_MAX_ITS) {
        a = newton_finish(s, RDC_NEWTON_LINEAR_FAILED, false);   // the coordinates have not moved
      } else {
        s.step = 1.0;
        s.measure = p.require_reduction ? 1 : 0;
        a = NEWTON_TRY_STEP;
      }
      break;
    case NEWTON_TRY_STEP:
    case NEWTON_HALVE:
      if (s.measure) I.assemblies++;
      I.last_step_norm = m.step_norm;
      I.last_solution_norm = m.solution_norm;
      if (!s.measure || m.residual < s.rn) {
        I.nonlinear_iterations = s.it + 1;
        s.measure = m.step_norm <= p.relative_step_tolerance * m.solution_norm ? 1 : 0;
        a = NEWTON_ACCEPT;
      } else {
        s.step *= 0.5;
        I.halvings++;
        s.measure = (p.require_reduction && !(s.step < 1e-3)) ? 1 : 0;
        a = NEWTON_HALVE;
      }
      break;
    case NEWTON_ACCEPT:
      if (s.measure) {
        I.assemblies++;
        I.last_residual = m.residual;
        a = std::isfinite(m.residual) ? newton_finish(s, RDC_NEWTON_CONVERGED_STEP, false) : newton_finish(s, RDC_NEWTON_NOT_FINITE, true);
      } else {
        s.it++;
        a = NEWTON_ASSEMBLE_FULL;
      }
      break;
    default:   // NEWTON_FINISH: nothing follows
      break;
  }
  s.last = a;
  return a;
}

// per Newton iteration of the last call (rdc_solid_newton_history); an iteration whose linear solve failed is listed with step 0
struct NewtonHistory {
  std::vector<double> residual, step;
  std::vector<int32_t> lin_its, lin_reason;
  void clear() { residual.clear(); step.clear(); lin_its.clear(); lin_reason.clear(); }
  void add(double r, double st, int32_t its, int32_t reason) { residual.push_back(r); step.push_back(st); lin_its.push_back(its); lin_reason.push_back(reason); }
};

}  // namespace rdc
#endif
