// g++ build of the host+device functions of the fp32 copy of the block ILU(0) factor (rdcfes_amd/csrc/rdc_solve.h:
// ilu_f32_offset, ilu_f32_node_floats, ilu_f32_offsets, ilu_place_f32, beside ilu_build, ilu_value_offset and ilu_factor_host) for
// tests/test_host_solve_ilu_f32.py, callable from ctypes; tests/host_solve_ilu_f32_main.cpp includes it and drives the same
// functions as a stand-alone program.
//
// The replay does on the CPU, through the offsets the kernels use, what a solve with "ilu_factor_bits" = 32 does on the device:
// the FP64 factor in the private layout, the rounding of its lower and upper blocks into the fp32 layout, and the two sweeps of one
// apply on the rounded blocks with everything else in FP64.
#include <cmath>
#include <cstring>
#include <limits>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace ilu_f32_replay {

struct Replay {
  int64_t n = 0;
  std::vector<int64_t> bptr;
  std::vector<int32_t> bcol;
  rdc::IluHost H;
  std::vector<int64_t> foff;
  std::vector<double> priv, uinv;   // the FP64 factor in the private layout, U_ii^-1
  std::vector<float> val32;         // the fp32 copy
  int64_t len(int64_t i) const { return H.nown.empty() ? bptr[(size_t)i + 1] - bptr[(size_t)i] : (int64_t)H.nown[(size_t)i]; }
};

// the public position (bcol ascends; the owned columns lead a row) of private position p of node i
inline int64_t public_block(const Replay& R, int64_t i, int64_t p) {
  const int32_t* r0 = R.bcol.data() + R.bptr[(size_t)i];
  return std::lower_bound(r0, r0 + R.len(i), R.H.pcol[(size_t)(R.bptr[(size_t)i] + p)]) - r0;
}

// ilu_build; 0 = fine
inline int build(Replay& R, int64_t n, const int64_t* bptr, const int32_t* bcol, bool ghosts) {
  R = Replay();
  R.n = n;
  R.bptr.assign(bptr, bptr + n + 1);
  R.bcol.assign(bcol, bcol + bptr[n]);
  int64_t where = -1;
  return rdc::ilu_build(n, bptr, bcol, R.H, &where, ghosts);
}

// The factor of A^ (val_in: per node [var a][owned block k][var b], the owned blocks of the nodes one behind the other), then the
// rounding: every entry through ilu_value_offset and ilu_f32_offset, the padding zeroed as k_ilu_round_f32 zeroes it, everything
// else of val32 left at the NaN it starts from.  val_out (the same layout as val_in) and uinv_out receive the FP64 factor.
// Returns the bad pivots; *overflow = entries that are finite in FP64 and not in fp32.
template <int NV>
int64_t factor_and_round(Replay& R, const double* val_in, double* val_out, double* uinv_out, int64_t* overflow) {
  const int64_t n = R.n;
  R.priv.assign((size_t)R.bptr[(size_t)n] * NV * NV, 0.0);
  R.uinv.assign((size_t)n * NV * NV, 0.0);
  auto move = [&](bool back) {
    int64_t o0 = 0;
    for (int64_t i = 0; i < n; i++) {
      const int64_t b0 = R.bptr[(size_t)i], own = R.len(i), nl = R.H.nlow[(size_t)i];
      for (int64_t p = 0; p < own; p++) {
        const int64_t k = public_block(R, i, p);
        for (int a = 0; a < NV; a++)
          for (int b = 0; b < NV; b++) {
            const int64_t pub = (int64_t)NV * NV * o0 + ((int64_t)a * own + k) * NV + b, pri = rdc::ilu_value_offset(b0, NV, own, nl, a, p, b);
            if (back) val_out[pub] = R.priv[(size_t)pri]; else R.priv[(size_t)pri] = val_in[pub];
          }
      }
      o0 += own;
    }
  };
  move(false);
  const int64_t bad = rdc::ilu_factor_host<NV>(n, R.bptr.data(), R.H, R.priv.data(), R.uinv.data());
  move(true);
  std::memcpy(uinv_out, R.uinv.data(), R.uinv.size() * sizeof(double));
  R.foff = rdc::ilu_f32_offsets(n, R.bptr.data(), R.H, NV);
  R.val32.assign((size_t)R.foff[(size_t)n], std::numeric_limits<float>::quiet_NaN());
  *overflow = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t b0 = R.bptr[(size_t)i], len = R.len(i), nl = R.H.nlow[(size_t)i], nup = len - nl - 1, f0 = R.foff[(size_t)i];
    for (int64_t p = 0; p < len; p++) {
      if (p == nl) continue;
      for (int a = 0; a < NV; a++)
        for (int b = 0; b < NV; b++) {
          const double v = R.priv[(size_t)rdc::ilu_value_offset(b0, NV, len, nl, a, p, b)];
          const float f = (float)v;
          *overflow += std::isfinite(v) && !std::isfinite(f);
          R.val32[(size_t)rdc::ilu_f32_offset(f0, NV, len, nl, a, p, b)] = f;
        }
    }
    const int64_t sl = rdc::f32_row_stride(NV, nl), su = rdc::f32_row_stride(NV, nup);
    for (int a = 0; a < NV; a++) {
      for (int64_t j = nl * NV; j < sl; j++) R.val32[(size_t)(f0 + a * sl + j)] = 0.0f;
      for (int64_t j = nup * NV; j < su; j++) R.val32[(size_t)(f0 + NV * sl + a * su + j)] = 0.0f;
    }
  }
  return bad;
}

// z = (LU)^-1 y on the rounded blocks: forward over the nodes in elimination order, backward in reverse, every value converted to
// double and fed to an fma in ascending position order
template <int NV>
void apply(const Replay& R, const double* y, double* z) {
  const std::vector<int32_t>& order = R.H.col.nodes;
  for (size_t at = 0; at < order.size(); at++) {
    const int64_t i = order[at], b0 = R.bptr[(size_t)i], len = R.len(i), nl = R.H.nlow[(size_t)i], f0 = R.foff[(size_t)i];
    for (int a = 0; a < NV; a++) {
      double s = 0.0;
      for (int64_t p = 0; p < nl; p++)
        for (int b = 0; b < NV; b++)
          s = std::fma((double)R.val32[(size_t)rdc::ilu_f32_offset(f0, NV, len, nl, a, p, b)], z[(int64_t)R.H.pcol[(size_t)(b0 + p)] * NV + b], s);
      z[i * NV + a] = y[i * NV + a] - s;
    }
  }
  for (size_t at = order.size(); at-- > 0;) {
    const int64_t i = order[at], b0 = R.bptr[(size_t)i], len = R.len(i), nl = R.H.nlow[(size_t)i], f0 = R.foff[(size_t)i];
    double t[NV];
    for (int a = 0; a < NV; a++) {
      double s = 0.0;
      for (int64_t p = nl + 1; p < len; p++)
        for (int b = 0; b < NV; b++)
          s = std::fma((double)R.val32[(size_t)rdc::ilu_f32_offset(f0, NV, len, nl, a, p, b)], z[(int64_t)R.H.pcol[(size_t)(b0 + p)] * NV + b], s);
      t[a] = z[i * NV + a] - s;
    }
    for (int a = 0; a < NV; a++) {
      double s = 0.0;
      for (int q = 0; q < NV; q++) s = std::fma(R.uinv[(size_t)((i * NV + a) * NV + q)], t[q], s);
      z[i * NV + a] = s;
    }
  }
}

}  // namespace ilu_f32_replay

#ifndef ILU_F32_NO_C_ENTRIES
namespace {
ilu_f32_replay::Replay g_R;
int g_nvar = 0;
}

extern "C" {

// ilu_build on a pattern (ghosts: columns >= n are ghost columns), kept for the calls below; returns its code
int shim_f32_build(int64_t n, const int64_t* bptr, const int32_t* bcol, int ghosts) { return ilu_f32_replay::build(g_R, n, bptr, bcol, ghosts != 0); }

// nown of the last build (n entries; the row lengths if the pattern has no ghost column) and nlow
void shim_f32_lists(int32_t* nown, int32_t* nlow) {
  for (int64_t i = 0; i < g_R.n; i++) { nown[i] = (int32_t)g_R.len(i); nlow[i] = g_R.H.nlow[(size_t)i]; }
}

// The fp32 layout of the last build for nvar unknowns: foff (n + 1 entries); off[nvar^2 * (bptr[i] + p) + a * nvar + b] =
// ilu_f32_offset of entry (node i, private position p, a, b), -1 at the diagonal position and at the positions of ghost columns;
// floats[i] = ilu_f32_node_floats of node i
void shim_f32_offsets(int nvar, int64_t* foff, int64_t* off, int64_t* floats) {
  const std::vector<int64_t> f = rdc::ilu_f32_offsets(g_R.n, g_R.bptr.data(), g_R.H, nvar);
  std::memcpy(foff, f.data(), f.size() * sizeof(int64_t));
  for (int64_t i = 0; i < g_R.n; i++) {
    const int64_t b0 = g_R.bptr[(size_t)i], len = g_R.len(i), nl = g_R.H.nlow[(size_t)i];
    floats[i] = rdc::ilu_f32_node_floats(nvar, len, nl);
    for (int64_t p = 0; p < g_R.bptr[(size_t)i + 1] - b0; p++)
      for (int a = 0; a < nvar; a++)
        for (int b = 0; b < nvar; b++)
          off[(int64_t)nvar * nvar * (b0 + p) + a * nvar + b] = p < len && p != nl ? rdc::ilu_f32_offset(f[(size_t)i], nvar, len, nl, a, p, b) : -1;
  }
}

// factor_and_round of the last build; returns the bad pivots, -1 for an nvar without kernels
int64_t shim_f32_factor(int nvar, const double* val_in, double* val_out, double* uinv, int64_t* overflow) {
  g_nvar = nvar;
  if (nvar == 1) return ilu_f32_replay::factor_and_round<1>(g_R, val_in, val_out, uinv, overflow);
  if (nvar == 3) return ilu_f32_replay::factor_and_round<3>(g_R, val_in, val_out, uinv, overflow);
  if (nvar == 5) return ilu_f32_replay::factor_and_round<5>(g_R, val_in, val_out, uinv, overflow);
  return -1;
}

// the fp32 copy of the last shim_f32_factor: copies it to `out` if given, returns its length in floats
int64_t shim_f32_values(float* out) {
  if (out && !g_R.val32.empty()) std::memcpy(out, g_R.val32.data(), g_R.val32.size() * sizeof(float));
  return (int64_t)g_R.val32.size();
}

// one apply on the rounded blocks of the last shim_f32_factor
void shim_f32_apply(const double* y, double* z) {
  if (g_nvar == 1) ilu_f32_replay::apply<1>(g_R, y, z);
  if (g_nvar == 3) ilu_f32_replay::apply<3>(g_R, y, z);
  if (g_nvar == 5) ilu_f32_replay::apply<5>(g_R, y, z);
}

// ilu_place_f32 of the last build: measures (base null), or places into an arena of `bytes` bytes; returns the bytes used, -1 if
// the arena is too small; at[0], at[1] = byte offsets of the offsets and of the floats
int64_t shim_f32_place(int nvar, char* base, int64_t bytes, int64_t* at) {
  const std::vector<int64_t> f = rdc::ilu_f32_offsets(g_R.n, g_R.bptr.data(), g_R.H, nvar);
  rdc::MgArena a;
  rdc::IluDev g;
  rdc::ilu_place_f32(f, a, g, [](void*, const void*, size_t) {});
  if (!base) return (int64_t)a.used;
  if (bytes < (int64_t)a.used) return -1;
  a = rdc::MgArena{base};
  rdc::ilu_place_f32(f, a, g, [](void* to, const void* list, size_t nb) { std::memcpy(to, list, nb); });
  at[0] = (const char*)g.foff - base; at[1] = (const char*)g.val32 - base;
  return (int64_t)a.used;
}

}
#endif
