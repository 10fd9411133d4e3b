// Stand-alone host program over rdcfes_amd/csrc/rdc_newton.h (no device, no Python), beside tests/host_newton_main.cpp: what
// rdc_solid_newton_dist decides on the host before anything is launched.  tests/test_host_newton_dist.py compares its output with a
// Python restatement; tools/asan_newton_dist.sh runs it under AddressSanitizer + UBSan.  Commands on standard input, one per line:
//   dispatch precond method          -> "dispatch entry needs"   (entry 0 rdc_solve_dist, 1 _mg, 2 _gmres; needs: 1 sized | 2 wide)
//   complete precond method mask     -> "complete 0|1"           (mask: which callbacks are not NULL; bit 0 exchange_begin, 1 exchange_end,
//                                                                 2 allreduce_sum, 3 exchange_sized_begin, 4 exchange_sized_end, 5 allreduce_sum_wide)
//   carve n_node n_owned             -> "carve n n_owned blocks u0 delta partials rec bytes n_delta send n_send"
//   carve_dist n_node n_owned n_send -> the same fields of newton_carve_dist
#include <cstdio>
#include <iostream>
#include <string>

#include "../rdcfes_amd/csrc/rdc_newton.h"

using namespace rdc;

static int cb_begin(void*, const double*, double*, void*) { return 0; }
static int cb_end(void*, void*) { return 0; }
static int cb_sum(void*, double*, int32_t, void*) { return 0; }
static int cb_sized(void*, const double*, double*, int32_t, const int64_t*, const int64_t*, void*) { return 0; }

static void print_work(const char* tag, const NewtonWork& w) {
  std::printf("%s %lld %lld %lld %lld %lld %lld %lld %zu %lld %lld %lld\n", tag, (long long)w.n, (long long)w.n_owned, (long long)w.blocks,
              (long long)w.u0, (long long)w.delta, (long long)w.partials, (long long)w.rec, w.bytes, (long long)w.n_delta, (long long)w.send,
              (long long)w.n_send);
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "dispatch") {
      long long precond, method;
      std::cin >> precond >> method;
      const NewtonDispatch d = newton_linear_dispatch((int32_t)precond, (int32_t)method);
      std::printf("dispatch %d %d\n", (int)d.entry, (int)d.needs);
    } else if (cmd == "complete") {
      long long precond, method, mask;
      std::cin >> precond >> method >> mask;
      rdc_solve_comm_wide c = rdc_solve_comm_wide();
      if (mask & 1) c.sized.base.exchange_begin = cb_begin;
      if (mask & 2) c.sized.base.exchange_end = cb_end;
      if (mask & 4) c.sized.base.allreduce_sum = cb_sum;
      if (mask & 8) c.sized.exchange_sized_begin = cb_sized;
      if (mask & 16) c.sized.exchange_sized_end = cb_end;
      if (mask & 32) c.allreduce_sum_wide = cb_sum;
      std::printf("complete %d\n", newton_comm_complete(c, newton_linear_dispatch((int32_t)precond, (int32_t)method)) ? 1 : 0);
    } else if (cmd == "carve") {
      long long n_node, n_owned;
      std::cin >> n_node >> n_owned;
      print_work("carve", newton_carve(n_node, n_owned));
    } else if (cmd == "carve_dist") {
      long long n_node, n_owned, n_send;
      std::cin >> n_node >> n_owned >> n_send;
      print_work("carve_dist", newton_carve_dist(n_node, n_owned, n_send));
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 1;
    }
  }
  return 0;
}
