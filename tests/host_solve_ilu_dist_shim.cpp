// g++ build of the block ILU(0) functions of rdcfes_amd/csrc/rdc_solve.h on a pattern WITH ghost columns (ilu_build with ghosts,
// ilu_value_offset over the owned positions, ilu_factor_node<NV, true> through ilu_factor_host, ilu_place with a ghost tail) for
// tests/test_host_solve_ilu_dist.py, callable from ctypes.  Values travel in the layout of a node-block CSR restricted to the owned
// columns, what rdc_solve_ilu_local_download returns: node i has own[i] blocks, [var a][block k][var b], the nodes one behind the other.
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

int64_t owned(int64_t i) { return g_H.nown.empty() ? g_bptr[(size_t)i + 1] - g_bptr[(size_t)i] : g_H.nown[(size_t)i]; }

// Factor of the owned square.  The private buffer has the slots of every block of the pattern; those of the ghost blocks are filled
// with a NaN of a payload of their own before the factorisation and compared bit for bit behind it: *disturbed = how many changed.
template <int NV>
int64_t factor(const double* val_in, double* val_out, double* uinv, int64_t* disturbed) {
  const int64_t n = (int64_t)g_bptr.size() - 1;
  uint64_t mark_bits = 0x7ff8000000c0ffeeull;
  double mark;
  std::memcpy(&mark, &mark_bits, sizeof(mark));
  std::vector<double> priv((size_t)g_bptr[(size_t)n] * NV * NV, mark);
  auto move = [&](bool back) {
    int64_t o0 = 0;
    for (int64_t i = 0; i < n; i++) {
      const int64_t b0 = g_bptr[(size_t)i], own = owned(i), nl = g_H.nlow[(size_t)i];
      for (int64_t p = 0; p < own; p++) {
        const int32_t* r0 = g_bcol.data() + b0;
        const int64_t k = std::lower_bound(r0, r0 + own, g_H.pcol[(size_t)(b0 + p)]) - r0;   // the owned columns lead the CSR row
        for (int a = 0; a < NV; a++)
          for (int b = 0; b < NV; b++) {
            const int64_t pub = (int64_t)NV * NV * o0 + ((int64_t)a * own + k) * NV + b, pri = rdc::ilu_value_offset(b0, NV, own, nl, a, p, b);
            if (back) val_out[pub] = priv[(size_t)pri]; else priv[(size_t)pri] = val_in[pub];
          }
      }
      o0 += own;
    }
  };
  move(false);
  const int64_t bad = rdc::ilu_factor_host<NV>(n, g_bptr.data(), g_H, priv.data(), uinv);
  move(true);
  *disturbed = 0;
  for (int64_t i = 0; i < n; i++)
    for (int64_t o = (int64_t)NV * NV * (g_bptr[(size_t)i] + owned(i)); o < (int64_t)NV * NV * g_bptr[(size_t)i + 1]; o++)
      *disturbed += std::memcmp(&priv[(size_t)o], &mark, sizeof(mark)) != 0;
  return bad;
}
}  // namespace

extern "C" {

// ilu_build on a pattern, with ghost columns allowed or (ghosts == 0) as the existing call; kept for the calls below
int shim_ilud_build(int64_t n, const int64_t* bptr, const int32_t* bcol, int ghosts, int64_t* where) {
  g_bptr.assign(bptr, bptr + n + 1);
  g_bcol.assign(bcol, bcol + bptr[n]);
  return ghosts ? rdc::ilu_build(n, bptr, bcol, g_H, where, true) : rdc::ilu_build(n, bptr, bcol, g_H, where);
}

// list `which` of the last build (0 colour, 1 cptr, 2 nodes, 3 pcol, 4 nlow, 5 nown): copies it to `out` if given, returns its length
int64_t shim_ilud_list(int which, void* out) {
  switch (which) {
    case 0: return give(g_H.col.colour, out);
    case 1: return give(g_H.col.cptr, out);
    case 2: return give(g_H.col.nodes, out);
    case 3: return give(g_H.pcol, out);
    case 4: return give(g_H.nlow, out);
    case 5: return give(g_H.nown, out);
  }
  return -1;
}

// off[nvar^2 * (bptr[i] + p) + a * nvar + b] = ilu_value_offset of entry (node i, OWNED position p, a, b), -1 at the positions of
// ghost columns; find[bptr[i] + p] = ilu_find of the column at an owned position in the owned part of its own row, -1 at a ghost's
void shim_ilud_offsets(int nvar, int64_t* off, int64_t* find) {
  const int64_t n = (int64_t)g_bptr.size() - 1;
  for (int64_t i = 0; i < n; i++) {
    const int64_t b0 = g_bptr[(size_t)i], len = g_bptr[(size_t)i + 1] - b0, own = owned(i), nl = g_H.nlow[(size_t)i];
    for (int64_t p = 0; p < len; p++) {
      find[b0 + p] = p < own ? rdc::ilu_find(g_H.pcol.data() + b0, own, g_H.col.colour.data(), g_H.pcol[(size_t)(b0 + p)]) : -1;
      for (int a = 0; a < nvar; a++)
        for (int b = 0; b < nvar; b++)
          off[(int64_t)nvar * nvar * (b0 + p) + a * nvar + b] = p < own ? rdc::ilu_value_offset(b0, nvar, own, nl, a, p, b) : -1;
    }
  }
}

// the factorisation of the owned square of the last build's pattern: val_in = A^ in the restricted layout, val_out = the factor in
// the same layout, uinv [n][nvar][nvar]; returns the pivots that could not be inverted, -1 for an nvar without kernels;
// *disturbed = slots of ghost blocks in the private buffer that the factorisation wrote
int64_t shim_ilud_factor(int nvar, const double* val_in, double* val_out, double* uinv, int64_t* disturbed) {
  if (nvar == 1) return factor<1>(val_in, val_out, uinv, disturbed);
  if (nvar == 3) return factor<3>(val_in, val_out, uinv, disturbed);
  if (nvar == 5) return factor<5>(val_in, val_out, uinv, disturbed);
  return -1;
}

// ilu_place of the last build with M p and M s sized for n_nodes: bytes[0], bytes[1] = the measured sizes of idx and val
void shim_ilud_place(int nvar, int64_t n_nodes, int64_t* bytes) {
  const int64_t n = (int64_t)g_bptr.size() - 1;
  rdc::MgArena a, v;
  rdc::IluDev g;
  rdc::ilu_place(g_H, nvar, n, g_bptr[(size_t)n], a, v, g, [](void*, const void*, size_t) {}, n_nodes);
  bytes[0] = (int64_t)a.used; bytes[1] = (int64_t)v.used;
}

}
