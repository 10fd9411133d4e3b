// Stand-alone run of the partitioned form of the GMRES state of rdcfes_amd/csrc/rdc_solve.h (gmres_carve with n_nodes): no device, no
// Python, for tools/asan_solve_gmres_dist.sh (-fsanitize=address,undefined).  The state is carved out of a heap buffer of exactly
// gmres_carve(...).bytes; then the program does on the host what a cycle does to it across ranks: every basis slot is written over
// its owned entries AND its ghost tail (the exchange receives there), a step's j + 2 sums go into red, are "all-reduced" in place
// (two ranks: doubled) and feed the Givens step as k_gmres_advance does it, the partials are written for the last step, and the
// back substitution fills y -- so that the sanitizer sees every part touched to its last double.  Returns 0 if the parts tile the
// buffer, the tails do not reach the next slot, and the least-squares residual has the norm the last rotation claims.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {

double entry(int i, int j) { return (i == j ? 3.0 : 0.0) + std::sin(1.0 + 0.7 * i + 1.9 * j) + (i == j + 1 ? 1.5 : 0.0); }

int check(int nvar, int64_t n_owned, int64_t n_nodes, int m) {
  const size_t bytes = rdc::gmres_carve(nvar, n_owned, m, nullptr, n_nodes).bytes;
  double* base = (double*)std::malloc(bytes);   // exactly the state: an overrun is seen
  const rdc::GmresState G = rdc::gmres_carve(nvar, n_owned, m, base, n_nodes);
  const int64_t want_stride = n_nodes * nvar > 1 ? n_nodes * nvar : 1;
  if (G.bytes != bytes || (char*)G.rec + sizeof(rdc::GmresRec) != (char*)base + bytes || G.V != base || !G.red || G.stride != want_stride ||
      G.n != n_owned * nvar || G.H != G.V + (int64_t)(m + 1) * G.stride || G.partials != G.red + m + 2 || G.red != G.scal + rdc::GMRES_SCALARS ||
      G.basis_bytes != (size_t)(m + 1) * G.stride * sizeof(double)) {
    std::printf("restart %d: the parts do not tile the buffer\n", m);
    return 1;
  }
  std::memset(base, 0, bytes);
  for (int k = 0; k <= m; k++) {                       // slot k: owned entries, then the tail an exchange receives into
    double* v = G.V + (int64_t)k * G.stride;
    for (int64_t i = 0; i < G.n; i++) v[i] = 1.0 + k;
    for (int64_t i = G.n; i < n_nodes * nvar; i++) v[i] = -1.0 - k;
  }
  for (int k = 0; k <= m; k++) {                       // no tail ran into the next slot
    const double* v = G.V + (int64_t)k * G.stride;
    if ((G.n > 0 && v[0] != 1.0 + k) || (n_nodes * nvar > G.n && v[n_nodes * nvar - 1] != -1.0 - k)) { std::printf("restart %d: slot %d overlaps\n", m, k); return 1; }
  }
  const int ld = m + 1;
  const double beta = 2.0;
  G.g[0] = beta;
  for (int j = 0; j < m; j++) {
    for (int i = 0; i <= j + 1; i++) G.red[i] = 0.5 * entry(i, j);   // this rank's sums: h_0..j and, last, (w, w) -- here the entry below the diagonal
    for (int i = 0; i <= j + 1; i++) G.red[i] += G.red[i];           // the wide all-reduce over two equal ranks, in place, j + 2 doubles
    double* hcol = G.H + (int64_t)j * ld;
    for (int i = 0; i <= j; i++) { G.hpass[i] = G.red[i]; hcol[i] = G.red[i]; }
    hcol[j + 1] = G.red[j + 1];
    if (rdc::gmres_givens_step(j, hcol, G.R + (int64_t)j * ld, G.cs, G.sn, G.g)) { std::printf("restart %d: column %d was not taken\n", m, j); return 1; }
    G.scal[1] = 1.0 / hcol[j + 1];
  }
  G.red[m + 1] = 1.0;                                  // the spare double of red
  for (int64_t i = 0; i < G.partial_count; i++) G.partials[i] = 1.0;
  G.rec->est = std::fabs(G.g[m]);
  G.rec->overflow = 0;
  if (!rdc::gmres_back_substitute(ld, m, G.R, G.g, G.y)) { std::printf("restart %d: y is not finite\n", m); return 1; }
  double rn2 = 0.0;
  for (int i = 0; i <= m; i++) {
    double s = i == 0 ? -beta : 0.0;
    for (int j = (i > 0 ? i - 1 : 0); j < m; j++) s += G.H[(int64_t)j * ld + i] * G.y[j];
    rn2 += s * s;
  }
  const double err = std::fabs(std::sqrt(rn2) - G.rec->est);
  std::free(base);
  if (!(err <= 1e-12)) { std::printf("restart %d: |H y - beta e_0| differs from |g_m| by %g\n", m, err); return 1; }
  std::printf("restart %d (nvar %d, %lld owned of %lld nodes): %zu bytes, stride %lld, least-squares residual matches |g_m| to %.1e\n", m, nvar,
              (long long)n_owned, (long long)n_nodes, bytes, (long long)G.stride, err);
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += check(3, 343, 400, 1) + check(5, 729, 729, 2) + check(5, 300, 421, 30) + check(5, 1, 9, 128) + check(5, 0, 7, 30) + check(3, 0, 0, 4);
  if (rdc::GMRES_WIDE_MAX != rdc::GMRES_MAX_RESTART + 2) bad++;
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
