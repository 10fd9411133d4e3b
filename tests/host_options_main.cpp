// Stand-alone driver of rdcfes_amd/csrc/rdc_options.h and rdc_solve_state.h for a sanitizer build (tools/asan_options.sh): every
// key of both tables with values around each rule's edges, unknown and over-long keys, message buffers down to one byte, and the
// validity rule over every entry, preconditioner and outcome.  Prints "ok" and returns 0.
#include <climits>
#include <string>

#include "../rdcfes_amd/csrc/rdc_options.h"
#include "../rdcfes_amd/csrc/rdc_solve_state.h"

static bool same(const rdc::Options& a, const rdc::Options& b) {
#define SAME(name, type, def, check, store) if (a.name != b.name) return false;
  RDC_OPTIONS(SAME)
  return true;
}

static bool same(const rdc::SolveOptions& a, const rdc::SolveOptions& b) {
  RDC_SOLVE_OPTIONS(SAME)
#undef SAME
  return true;
}

// every key of one table with every value; a refusal leaves the struct and writes a message that fits
template <class O, class Set>
static int drive(const char* const* keys, int n, Set set, int* accepted, int* refused) {
  const int values[] = {INT_MIN, -3, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 30, 31, 32, 62, 64, 99, 128, 129, 256, 600, 1999, 2000, 54000, INT_MAX};
  for (size_t errlen : {(size_t)512, (size_t)16, (size_t)1}) {
    std::string err(errlen, '\0');
    O o;
    for (int k = 0; k < n; k++)
      for (int v : values) {
        const O before = o;
        const int rc = set(o, keys[k], v, &err[0], errlen);
        if (rc == RDC_OK) { ++*accepted; continue; }
        ++*refused;
        if (rc != RDC_ERR_INVALID || !same(before, o) || std::strlen(err.c_str()) >= errlen) return 1;
      }
    const std::string longkey(4000, 'k');
    for (const char* key : {"", "slim", "kernel ", "mg_omega ", longkey.c_str()})
      if (set(o, key, 1, &err[0], errlen) != RDC_ERR_INVALID || std::strlen(err.c_str()) >= errlen) return 2;
  }
  return 0;
}

// the rule over every call and outcome: a flag is only ever set by a call that ran to its end
static int drive_validity() {
  int n = 0;
  for (int entry = 0; entry <= (int)rdc::SolveEntry::DIST_PLAN; entry++)
    for (int precond = RDC_PRECOND_NONE; precond <= RDC_PRECOND_ILU0_LOCAL; precond++)
      for (int bits = 0; bits < 256; bits++) {
        rdc::SolveCall call{(rdc::SolveEntry)entry, precond, (bits & 1) != 0, (bits & 2) != 0};
        rdc::SolveOutcome o;
        o.ran = bits & 4; o.comm_failed = bits & 8; o.bad_blocks = bits & 16 ? INT_MAX : 0; o.matrix_bits = bits & 32 ? 32 : 64;
        o.reason = bits & 64 ? RDC_SOLVE_BAD_DIAGONAL : RDC_SOLVE_CONVERGED;
        rdc::SolveValid v;
        if (bits & 128) v.f32_copy = v.mg_values = v.ilu_factored = v.gmres_solved = true;
        const rdc::SolveValid before = v;
        rdc::solve_valid_enter(v, call.entry);
        rdc::solve_valid_begin(v, call);
        rdc::solve_valid_leave(v, call, o);
        const bool ended = o.ran && !o.comm_failed;
        if (!ended && ((v.f32_copy && !before.f32_copy) || v.mg_values || (v.ilu_factored && !before.ilu_factored) ||
                       (v.gmres_solved && !before.gmres_solved)))
          return -1;
        n++;
      }
  return n;
}

int main() {
  int n = 0, ns = 0, refused = 0, accepted = 0;
  const char* const* keys = rdc::option_keys(&n);
  int rc = drive<rdc::Options>(keys, n, [](rdc::Options& o, const char* k, int v, char* e, size_t l) { return rdc::options_set(o, k, v, e, l); },
                               &accepted, &refused);
  if (rc) return rc;
  const char* const* skeys = rdc::solve_option_keys(&ns);
  rc = drive<rdc::SolveOptions>(skeys, ns, [](rdc::SolveOptions& o, const char* k, int v, char* e, size_t l) { return rdc::solve_options_set(o, k, v, e, l); },
                                &accepted, &refused);
  if (rc) return rc + 2;
  for (int k = 0; k < n; k++) if (rdc::solve_option_known(keys[k])) return 5;
  for (int k = 0; k < ns; k++) if (!rdc::solve_option_known(skeys[k])) return 6;
  const int calls = drive_validity();
  if (calls < 0) return 7;
  std::printf("ok: %d + %d keys, %d values accepted, %d refused, %d calls under the validity rule\n", n, ns, accepted, refused, calls);
  return n == 28 && ns == 7 ? 0 : 3;
}
