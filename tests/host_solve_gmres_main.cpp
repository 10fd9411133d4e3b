// Stand-alone run of the GMRES functions of rdcfes_amd/csrc/rdc_solve.h (gmres_carve, gmres_givens_step, gmres_back_substitute):
// no device, no Python, for tools/asan_solve_gmres.sh (-fsanitize=address,undefined).  For each restart length the state is carved out of a
// heap buffer of exactly gmres_carve(...).bytes, a Hessenberg matrix is written column after column into H, every column goes
// through the Givens step into R, cs, sn and g as k_gmres_finalize does it, and the back substitution fills y, so that the sanitizer
// sees every read and write those functions make inside the carved parts.  Returns 0 if the least-squares residual H y - beta e_0
// has the norm the last rotation claims, the parts tile the buffer, and the flagged cases leave g alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {

double entry(int i, int j) { return (i == j ? 3.0 : 0.0) + std::sin(1.0 + 0.7 * i + 1.9 * j) + (i == j + 1 ? 1.5 : 0.0); }

int check(int nvar, int64_t n_owned, int m) {
  const size_t bytes = rdc::gmres_carve(nvar, n_owned, m, nullptr).bytes;
  double* base = (double*)std::malloc(bytes);   // exactly the state: an overrun is seen
  const rdc::GmresState G = rdc::gmres_carve(nvar, n_owned, m, base);
  if (G.bytes != bytes || (char*)G.rec + sizeof(rdc::GmresRec) != (char*)base + bytes || G.V != base) {
    std::printf("restart %d: the parts do not tile the buffer\n", m);
    return 1;
  }
  std::memset(base, 0, bytes);
  const int ld = m + 1;
  const double beta = 2.0;
  G.g[0] = beta;
  for (int j = 0; j < m; j++) {
    double* hcol = G.H + (int64_t)j * ld;
    for (int i = 0; i <= j + 1; i++) hcol[i] = entry(i, j);
    if (rdc::gmres_givens_step(j, hcol, G.R + (int64_t)j * ld, G.cs, G.sn, G.g)) { std::printf("restart %d: column %d was not taken\n", m, j); return 1; }
  }
  G.rec->est = std::fabs(G.g[m]);
  if (!rdc::gmres_back_substitute(ld, m, G.R, G.g, G.y)) { std::printf("restart %d: y is not finite\n", m); return 1; }
  double rn2 = 0.0;
  for (int i = 0; i <= m; i++) {
    double s = i == 0 ? -beta : 0.0;
    for (int j = (i > 0 ? i - 1 : 0); j < m; j++) s += G.H[(int64_t)j * ld + i] * G.y[j];
    rn2 += s * s;
  }
  const double err = std::fabs(std::sqrt(rn2) - G.rec->est);
  // a column with a non-finite entry, and a zero column: flagged, g untouched
  int fail = 0;
  if (m >= 2) {
    const double g0 = G.g[1], g1 = G.g[2];
    double* hcol = G.H + (int64_t)1 * ld;
    const double keep = hcol[0];
    hcol[0] = NAN;
    fail += rdc::gmres_givens_step(1, hcol, G.R + (int64_t)1 * ld, G.cs, G.sn, G.g) != rdc::GMRES_NOT_FINITE;
    hcol[0] = keep;
    fail += G.g[1] != g0 || G.g[2] != g1;
  }
  {
    double* hcol = G.H;
    hcol[0] = hcol[1] = 0.0;
    const double g0 = G.g[0];
    fail += rdc::gmres_givens_step(0, hcol, G.R, G.cs, G.sn, G.g) != rdc::GMRES_SINGULAR || G.g[0] != g0;
  }
  std::free(base);
  if (!(err <= 1e-12) || fail) { std::printf("restart %d: |H y - beta e_0| differs from |g_m| by %g, %d flag checks failed\n", m, err, fail); return 1; }
  std::printf("restart %d (nvar %d, %lld nodes): %zu bytes, least-squares residual matches |g_m| to %.1e\n", m, nvar, (long long)n_owned, bytes, err);
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += check(3, 343, 1) + check(5, 729, 2) + check(3, 343, 30) + check(5, 1, 128) + check(5, 0, 30);
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
