// Stand-alone run of the host+device functions of the fp32 copy of the block ILU(0) factor (rdcfes_amd/csrc/rdc_solve.h:
// ilu_f32_offset, ilu_f32_node_floats, ilu_f32_offsets, ilu_place_f32) through the replay of tests/host_solve_ilu_f32_shim.cpp, for
// tests/test_host_solve_ilu_f32.py to build with AddressSanitizer and UBSan: a block-tridiagonal and an arrow matrix, and a
// block-tridiagonal one whose last rows couple to ghost columns, for nvar 1, 3 and 5.  Every offset is checked to lie inside its
// node, every float of the copy to have been written (none keeps the NaN it starts from), the padding to be zero, and one apply
// on the rounded blocks to be an fp32 perturbation of the apply on the FP64 blocks.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "host_solve_ilu_f32_shim.cpp"

namespace {
using ilu_f32_replay::Replay;

struct Pattern {
  int64_t n = 0;
  std::vector<int64_t> bptr;
  std::vector<int32_t> bcol;
  bool ghosts = false;
};

Pattern tridiagonal(int64_t n, int64_t first_ghosted) {   // rows >= first_ghosted get two ghost columns each
  Pattern P;
  P.n = n; P.bptr.push_back(0); P.ghosts = first_ghosted < n;
  for (int64_t i = 0; i < n; i++) {
    for (int64_t j = i - 1; j <= i + 1; j++)
      if (j >= 0 && j < n) P.bcol.push_back((int32_t)j);
    if (i >= first_ghosted) { P.bcol.push_back((int32_t)(n + (i - first_ghosted))); P.bcol.push_back((int32_t)(n + 40 + i)); }
    P.bptr.push_back((int64_t)P.bcol.size());
  }
  return P;
}

Pattern arrow(int64_t n) {   // n - 1 leaves coupled to the last node only
  Pattern P;
  P.n = n; P.bptr.push_back(0);
  for (int64_t i = 0; i < n; i++) {
    if (i < n - 1) { P.bcol.push_back((int32_t)i); P.bcol.push_back((int32_t)(n - 1)); }
    else for (int64_t j = 0; j < n; j++) P.bcol.push_back((int32_t)j);
    P.bptr.push_back((int64_t)P.bcol.size());
  }
  return P;
}

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } \
  } while (0)

template <int NV>
void run(const Pattern& P, unsigned seed) {
  Replay R;
  CHECK(ilu_f32_replay::build(R, P.n, P.bptr.data(), P.bcol.data(), P.ghosts) == 0);
  CHECK(P.ghosts == !R.H.nown.empty());
  // A^: random blocks, identity-dominated diagonal (compact owned layout)
  int64_t owned = 0;
  for (int64_t i = 0; i < P.n; i++) owned += R.len(i);
  std::vector<double> val((size_t)owned * NV * NV), fac(val.size()), uinv((size_t)P.n * NV * NV);
  unsigned s = seed;
  auto rnd = [&] { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) - 0.5; };
  int64_t o0 = 0;
  for (int64_t i = 0; i < P.n; i++) {
    const int64_t own = R.len(i);
    for (int64_t k = 0; k < own; k++)
      for (int a = 0; a < NV; a++)
        for (int b = 0; b < NV; b++)
          val[(size_t)(NV * NV * o0 + (a * own + k) * NV + b)] = 0.3 * rnd() + (P.bcol[(size_t)(P.bptr[(size_t)i] + k)] == i && a == b ? 1.0 : 0.0);
    o0 += own;
  }
  int64_t overflow = -1;
  CHECK(ilu_f32_replay::factor_and_round<NV>(R, val.data(), fac.data(), uinv.data(), &overflow) == 0);
  CHECK(overflow == 0);
  // the layout: every (a, p != nlow, b) of the owned positions exactly once, inside the node, rows at multiples of 4 floats
  std::set<int64_t> seen;
  for (int64_t i = 0; i < P.n; i++) {
    const int64_t len = R.len(i), nl = R.H.nlow[(size_t)i], f0 = R.foff[(size_t)i];
    CHECK(f0 % 4 == 0 && R.foff[(size_t)i + 1] - f0 == rdc::ilu_f32_node_floats(NV, len, nl));
    for (int64_t p = 0; p < len; p++) {
      if (p == nl) continue;
      for (int a = 0; a < NV; a++) {
        CHECK(rdc::ilu_f32_offset(f0, NV, len, nl, a, p < nl ? 0 : nl + 1, 0) % 4 == 0);
        for (int b = 0; b < NV; b++) {
          const int64_t o = rdc::ilu_f32_offset(f0, NV, len, nl, a, p, b);
          CHECK(o >= f0 && o < R.foff[(size_t)i + 1]);
          CHECK(seen.insert(o).second);
        }
      }
    }
  }
  int64_t padding = 0;
  for (int64_t o = 0; o < R.foff[(size_t)P.n]; o++) {
    CHECK(R.val32[(size_t)o] == R.val32[(size_t)o]);   // written: no NaN left
    if (!seen.count(o)) { CHECK(R.val32[(size_t)o] == 0.0f); padding++; }
  }
  CHECK((int64_t)seen.size() + padding == R.foff[(size_t)P.n]);
  // the placement into an arena of exactly the measured size
  rdc::MgArena a;
  rdc::IluDev g;
  rdc::ilu_place_f32(R.foff, a, g, [](void*, const void*, size_t) {});
  std::vector<char> arena(a.used + rdc::MG_ALIGN);
  char* base = arena.data() + (rdc::MG_ALIGN - (size_t)((uintptr_t)arena.data() % rdc::MG_ALIGN)) % rdc::MG_ALIGN;
  const size_t measured = a.used;
  a = rdc::MgArena{base};
  rdc::ilu_place_f32(R.foff, a, g, [](void* to, const void* list, size_t nb) { std::memcpy(to, list, nb); });
  CHECK(a.used == measured && (const char*)g.foff == base && std::memcmp(g.foff, R.foff.data(), R.foff.size() * sizeof(int64_t)) == 0);
  CHECK((uintptr_t)g.val32 % 16 == 0 && (const char*)(g.val32 + std::max<int64_t>(R.foff[(size_t)P.n], 1)) <= base + measured);
  std::memcpy(g.val32, R.val32.data(), R.val32.size() * sizeof(float));
  // one apply on the rounded blocks against the same sweeps on the FP64 blocks
  std::vector<double> y((size_t)P.n * NV), z(y.size()), w(y.size());
  for (double& v : y) v = rnd();
  ilu_f32_replay::apply<NV>(R, y.data(), z.data());
  const Replay& E = R;   // the same sweeps on the FP64 blocks of the private layout
  const std::vector<int32_t>& order = R.H.col.nodes;
  for (size_t at = 0; at < order.size(); at++) {
    const int64_t i = order[at], b0 = R.bptr[(size_t)i], len = R.len(i), nl = R.H.nlow[(size_t)i];
    for (int a2 = 0; a2 < NV; a2++) {
      double t = 0.0;
      for (int64_t p = 0; p < nl; p++)
        for (int b = 0; b < NV; b++) t += E.priv[(size_t)rdc::ilu_value_offset(b0, NV, len, nl, a2, p, b)] * w[(size_t)(R.H.pcol[(size_t)(b0 + p)] * NV + b)];
      w[(size_t)(i * NV + a2)] = y[(size_t)(i * NV + a2)] - t;
    }
  }
  for (size_t at = order.size(); at-- > 0;) {
    const int64_t i = order[at], b0 = R.bptr[(size_t)i], len = R.len(i), nl = R.H.nlow[(size_t)i];
    double t[NV];
    for (int a2 = 0; a2 < NV; a2++) {
      t[a2] = w[(size_t)(i * NV + a2)];
      for (int64_t p = nl + 1; p < len; p++)
        for (int b = 0; b < NV; b++) t[a2] -= E.priv[(size_t)rdc::ilu_value_offset(b0, NV, len, nl, a2, p, b)] * w[(size_t)(R.H.pcol[(size_t)(b0 + p)] * NV + b)];
    }
    for (int a2 = 0; a2 < NV; a2++) {
      double u = 0.0;
      for (int q = 0; q < NV; q++) u += R.uinv[(size_t)((i * NV + a2) * NV + q)] * t[q];
      w[(size_t)(i * NV + a2)] = u;
    }
  }
  double d2 = 0.0, w2 = 0.0;
  for (size_t k = 0; k < z.size(); k++) { CHECK(std::isfinite(z[k])); d2 += (z[k] - w[k]) * (z[k] - w[k]); w2 += w[k] * w[k]; }
  const double rel = std::sqrt(d2 / w2);
  CHECK(rel > 1e-10 && rel < 1e-6);
}

template <int NV>
void all(unsigned seed) {
  run<NV>(tridiagonal(37, 37), seed);
  run<NV>(arrow(23), seed + 1);
  run<NV>(tridiagonal(29, 17), seed + 2);
}
}  // namespace

int main() {
  all<1>(13);
  all<3>(11);
  all<5>(12);
  std::printf("ok: fp32 layout, rounding and apply on 9 patterns\n");
  return 0;
}
