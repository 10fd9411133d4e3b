// Stand-alone host program over rdcfes_amd/csrc/rdc_newton.h (no device, no Python): drives newton_next with scripted norms and
// reports newton_carve and newton_check_params.  tests/test_host_newton.py compares its output with a Python restatement;
// tools/asan_newton.sh runs it under AddressSanitizer + UBSan.  Commands on standard input, one per line:
//   check max req rel_step rel_res abs_res lin_rel lin_abs lin_max precond mixed       -> "check 0|1"
//   carve n_node n_owned                                                                  -> "carve n n_owned blocks u0 delta partials rec bytes"
//   run max req rel_step rel_res abs_res K, then K lines "residual step_norm solution_norm lin_reason lin_its": what the
//   actions measure, one line per action executed                                         -> "act ..." per action, then "info ..."
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../rdcfes_amd/csrc/rdc_newton.h"

using namespace rdc;

static double num(std::istream& in) {
  std::string t;
  in >> t;
  return std::strtod(t.c_str(), nullptr);   // takes nan and inf
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "check") {
      rdc_solid_newton_params p = rdc_solid_newton_params();
      p.max_nonlinear_iterations = (int32_t)num(std::cin); p.require_reduction = (int32_t)num(std::cin);
      p.relative_step_tolerance = num(std::cin); p.relative_residual_tolerance = num(std::cin); p.absolute_residual_tolerance = num(std::cin);
      p.linear.rel_tol = num(std::cin); p.linear.abs_tol = num(std::cin); p.linear.max_its = (int32_t)num(std::cin);
      p.linear.precond = (int32_t)num(std::cin); p.mixed = (int32_t)num(std::cin);
      std::printf("check %d\n", newton_check_params(p) == nullptr ? 1 : 0);
    } else if (cmd == "carve") {
      const int64_t n_node = (int64_t)num(std::cin), n_owned = (int64_t)num(std::cin);
      const NewtonWork w = newton_carve(n_node, n_owned);
      std::printf("carve %lld %lld %lld %lld %lld %lld %lld %zu\n", (long long)w.n, (long long)w.n_owned, (long long)w.blocks, (long long)w.u0,
                  (long long)w.delta, (long long)w.partials, (long long)w.rec, w.bytes);
    } else if (cmd == "constants") {
      std::printf("constants %d %d %d %zu\n", NEWTON_CHUNK, NEWTON_ALIGN, NEWTON_REC_DOUBLES, sizeof(NewtonRec));
    } else if (cmd == "sizes") {
      std::printf("sizes %zu %zu\n", sizeof(rdc_solid_newton_params), sizeof(rdc_solid_newton_info));
    } else if (cmd == "run") {
      rdc_solid_newton_params p = rdc_solid_newton_params();
      p.max_nonlinear_iterations = (int32_t)num(std::cin); p.require_reduction = (int32_t)num(std::cin);
      p.relative_step_tolerance = num(std::cin); p.relative_residual_tolerance = num(std::cin); p.absolute_residual_tolerance = num(std::cin);
      int left = (int)num(std::cin);
      NewtonState s;
      NewtonNorms m;
      for (int guard = 0; guard < 100000; guard++) {
        const NewtonAction a = newton_next(p, s, m);
        std::printf("act %d measure %d restore %d step %.17g it %d\n", (int)a, s.measure, s.restore, s.step, s.it);
        if (a == NEWTON_FINISH) break;
        if (left-- <= 0) { std::printf("error script exhausted\n"); return 2; }
        m = NewtonNorms();
        m.residual = num(std::cin); m.step_norm = num(std::cin); m.solution_norm = num(std::cin);
        m.linear_reason = (int32_t)num(std::cin); m.linear_iterations = (int32_t)num(std::cin);
      }
      while (left-- > 0) for (int k = 0; k < 5; k++) (void)num(std::cin);   // what a run that ended early did not consume
      const rdc_solid_newton_info& I = s.info;
      std::printf("info %d %d %d %d %d %d %.17g %.17g %.17g %.17g\n", I.reason, I.nonlinear_iterations, I.linear_iterations, I.assemblies,
                  I.halvings, I.last_linear_reason, I.first_residual, I.last_residual, I.last_step_norm, I.last_solution_norm);
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 1;
    }
  }
  return 0;
}
