// g++ build of the host-only headers behind the linear-solve entries of the C-ABI for tests/test_host_solve_state.py: the table of
// solver settings (rdc_options.h, RDC_SOLVE_OPTIONS) and the validity rule of the cached artefacts (rdc_solve_state.h), callable
// from ctypes without a device.
#include "../rdcfes_amd/csrc/rdc_options.h"
#include "../rdcfes_amd/csrc/rdc_solve_state.h"

extern "C" {

void* shim_solve_options_new() { return new rdc::SolveOptions(); }
void shim_solve_options_delete(void* o) { delete static_cast<rdc::SolveOptions*>(o); }

int shim_solve_options_set(void* o, const char* key, int value, char* err, int errlen) {
  return rdc::solve_options_set(*static_cast<rdc::SolveOptions*>(o), key, value, err, (size_t)errlen);
}

// stored value of a key; *found = 0: no such member
int shim_solve_options_get(const void* o, const char* key, int* found) {
  const rdc::SolveOptions& opt = *static_cast<const rdc::SolveOptions*>(o);
  *found = 1;
#define SHIM_GET(name, type, def, check, store) \
  if (!std::strcmp(key, #name)) return (int)opt.name;
  RDC_SOLVE_OPTIONS(SHIM_GET)
#undef SHIM_GET
  *found = 0;
  return 0;
}

int shim_solve_option_count() { int n = 0; rdc::solve_option_keys(&n); return n; }
const char* shim_solve_option_key(int i) { int n = 0; return rdc::solve_option_keys(&n)[i]; }
int shim_solve_option_known(const char* key) { return rdc::solve_option_known(key) ? 1 : 0; }

// a key of the solver table offered to the tuning table
int shim_tuning_options_set(const char* key, int value, char* err, int errlen) {
  rdc::Options o;
  return rdc::options_set(o, key, value, err, (size_t)errlen);
}

// One call under the rule.  flags: f32_copy, mg_values, ilu_factored, gmres_solved, gmres_restart, gmres_cycles (in and out).
// stage 0: refused after entry (enter only); 1: a view failed (enter, begin); 2: the call left (enter, begin, leave with
// outcome = ran, comm_failed, bad_blocks, matrix_bits, reason, gmres_restart, gmres_cycles)
void shim_valid_apply(int* flags, int entry, int precond, int mixed, int gmres, int stage, const int* outcome) {
  rdc::SolveValid v;
  v.f32_copy = flags[0] != 0; v.mg_values = flags[1] != 0; v.ilu_factored = flags[2] != 0; v.gmres_solved = flags[3] != 0;
  v.gmres_restart = flags[4]; v.gmres_cycles = flags[5];
  rdc::SolveCall call{(rdc::SolveEntry)entry, precond, mixed != 0, gmres != 0};
  rdc::solve_valid_enter(v, call.entry);
  if (stage >= 1) rdc::solve_valid_begin(v, call);
  if (stage >= 2) {
    rdc::SolveOutcome o;
    o.ran = outcome[0] != 0; o.comm_failed = outcome[1] != 0; o.bad_blocks = outcome[2]; o.matrix_bits = outcome[3]; o.reason = outcome[4];
    o.gmres_restart = outcome[5]; o.gmres_cycles = outcome[6];
    rdc::solve_valid_leave(v, call, o);
  }
  flags[0] = v.f32_copy; flags[1] = v.mg_values; flags[2] = v.ilu_factored; flags[3] = v.gmres_solved;
  flags[4] = v.gmres_restart; flags[5] = v.gmres_cycles;
}

}
