// g++ build of the host+device functions of the block ILU(0) (rdcfes_amd/csrc/rdc_solve.h: ilu_build, ilu_value_offset, ilu_find,
// ilu_factor_node through ilu_factor_host, ilu_place) for tests/test_host_solve_ilu.py, callable from ctypes.
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {
rdc::IluHost g_H;
std::vector<int64_t> g_bptr;
std::vector<int32_t> g_bcol;

template <class T>
int64_t give(const std::vector<T>& v, void* out) {
  if (out && !v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
  return (int64_t)v.size();
}

// public position (bcol ascends) of private position p of node i
int64_t public_block(int64_t i, int64_t p) {
  const int32_t* r0 = g_bcol.data() + g_bptr[(size_t)i];
  const int32_t* r1 = g_bcol.data() + g_bptr[(size_t)i + 1];
  return std::lower_bound(r0, r1, g_H.pcol[(size_t)(g_bptr[(size_t)i] + p)]) - r0;
}

// factor of A^ (val_in: public layout, already scaled) -> val_out (public layout), uinv; returns the bad pivots
template <int NV>
int64_t factor(const double* val_in, double* val_out, double* uinv) {
  const int64_t n = (int64_t)g_bptr.size() - 1;
  std::vector<double> priv((size_t)g_bptr[(size_t)n] * NV * NV);
  auto move = [&](bool back) {
    for (int64_t i = 0; i < n; i++) {
      const int64_t b0 = g_bptr[(size_t)i], len = g_bptr[(size_t)i + 1] - b0, nl = g_H.nlow[(size_t)i];
      for (int64_t p = 0; p < len; p++) {
        const int64_t k = public_block(i, p);
        for (int a = 0; a < NV; a++)
          for (int b = 0; b < NV; b++) {
            const int64_t pub = rdc::csr_value_offset(g_bptr.data(), NV, i, a, k, b), pri = rdc::ilu_value_offset(b0, NV, len, nl, a, p, b);
            if (back) val_out[pub] = priv[(size_t)pri]; else priv[(size_t)pri] = val_in[pub];
          }
      }
    }
  };
  move(false);
  const int64_t bad = rdc::ilu_factor_host<NV>(n, g_bptr.data(), g_H, priv.data(), uinv);
  move(true);
  return bad;
}
}  // namespace

extern "C" {

// ilu_build on a pattern, kept for the calls below; returns its code, *where as it sets it
int shim_ilu_build(int64_t n, const int64_t* bptr, const int32_t* bcol, int64_t* where) {
  g_bptr.assign(bptr, bptr + n + 1);
  g_bcol.assign(bcol, bcol + bptr[n]);
  return rdc::ilu_build(n, bptr, bcol, g_H, where);
}

// list `which` of the last build (0 colour, 1 cptr, 2 nodes, 3 pcol, 4 nlow): copies it to `out` if given, returns its length
int64_t shim_ilu_list(int which, void* out) {
  switch (which) {
    case 0: return give(g_H.col.colour, out);
    case 1: return give(g_H.col.cptr, out);
    case 2: return give(g_H.col.nodes, out);
    case 3: return give(g_H.pcol, out);
    case 4: return give(g_H.nlow, out);
  }
  return -1;
}

// The private layout of the last build for nvar unknowns: off[nvar^2 * (bptr[i] + p) + a * nvar + b] = ilu_value_offset of entry
// (node i, position p, a, b), for every node and position; find[bptr[i] + p] = ilu_find of the column at that position in its own row
void shim_ilu_offsets(int nvar, int64_t* off, int64_t* find) {
  const int64_t n = (int64_t)g_bptr.size() - 1;
  for (int64_t i = 0; i < n; i++) {
    const int64_t b0 = g_bptr[(size_t)i], len = g_bptr[(size_t)i + 1] - b0, nl = g_H.nlow[(size_t)i];
    for (int64_t p = 0; p < len; p++) {
      find[b0 + p] = rdc::ilu_find(g_H.pcol.data() + b0, len, g_H.col.colour.data(), g_H.pcol[(size_t)(b0 + p)]);
      for (int a = 0; a < nvar; a++)
        for (int b = 0; b < nvar; b++) off[(int64_t)nvar * nvar * (b0 + p) + a * nvar + b] = rdc::ilu_value_offset(b0, nvar, len, nl, a, p, b);
    }
  }
}

// ilu_find of a column the row does not have (node j in the row of node i): -1 expected
int64_t shim_ilu_find(int64_t i, int32_t j) {
  const int64_t b0 = g_bptr[(size_t)i];
  return rdc::ilu_find(g_H.pcol.data() + b0, g_bptr[(size_t)i + 1] - b0, g_H.col.colour.data(), j);
}

// the factorisation of the last build's pattern: val_in = A^ in the layout of the CSR values, val_out = the factor in the same
// layout, uinv [n][nvar][nvar]; returns the number of pivots that could not be inverted, -1 for an nvar without kernels
int64_t shim_ilu_factor(int nvar, const double* val_in, double* val_out, double* uinv) {
  if (nvar == 1) return factor<1>(val_in, val_out, uinv);
  if (nvar == 3) return factor<3>(val_in, val_out, uinv);
  if (nvar == 5) return factor<5>(val_in, val_out, uinv);
  return -1;
}

// ilu_place of the last build: measures, then places into the two arenas (null: measure only).  bytes[0], bytes[1] = the measured
// sizes of idx and val; off[0 .. 4) = byte offsets of pcol, nlow, colour, nodes in idx, off[4 .. 8) = of val, uinv, ph, sh in val.
// Returns 0, -1 if an arena is too small, -2 if the two passes disagree.
int shim_ilu_place(int nvar, char* idx, int64_t idx_bytes, char* val, int64_t val_bytes, int64_t* bytes, int64_t* off) {
  const int64_t n = (int64_t)g_bptr.size() - 1;
  rdc::MgArena a, v;
  rdc::IluDev g;
  rdc::ilu_place(g_H, nvar, n, g_bptr[(size_t)n], a, v, g, [](void*, const void*, size_t) {});
  bytes[0] = (int64_t)a.used; bytes[1] = (int64_t)v.used;
  if (!idx || !val) return 0;
  if (idx_bytes < bytes[0] || val_bytes < bytes[1]) return -1;
  a = rdc::MgArena{idx}; v = rdc::MgArena{val};
  rdc::ilu_place(g_H, nvar, n, g_bptr[(size_t)n], a, v, g, [](void* at, const void* list, size_t nb) { std::memcpy(at, list, nb); });
  if ((int64_t)a.used != bytes[0] || (int64_t)v.used != bytes[1] || g.n_colours != g_H.col.n_colours() || g.cptr_host != g_H.col.cptr.data()) return -2;
  off[0] = (const char*)g.pcol - idx; off[1] = (const char*)g.nlow - idx; off[2] = (const char*)g.colour - idx; off[3] = (const char*)g.nodes - idx;
  off[4] = (const char*)g.val - val; off[5] = (const char*)g.uinv - val; off[6] = (const char*)g.ph - val; off[7] = (const char*)g.sh - val;
  return 0;
}

}
