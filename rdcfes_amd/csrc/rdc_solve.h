// rdc_solve.h — index arithmetic of the node-block CSR pattern and the inverse of a diagonal block, as the kernels of
// rdc_solve.hip use them.  Host+device like rdc_row.h, so that a CPU build can test exactly this code
// (tests/host_solve_shim.cpp); free of other headers of the library on purpose.  Further down: the host side of the
// aggregation multigrid (aggregates, coarse patterns, the lists of the Galerkin kernel; tests/host_solve_mg_shim.cpp) and
// the one statement of where a hierarchy lies on the device (MgDev, mg_place; tests/host_solve_mg_main.cpp), the colour lists of the
// Gauss-Seidel smoother (mg_colour, mg_gs_place; tests/host_solve_mg_gs_shim.cpp, tests/host_solve_mg_gs_main.cpp), and the hierarchy of a
// ghosted context, whose aggregates stay inside the partition (MgHalo, mg_dist_*; tests/host_solve_mg_dist_shim.cpp; its
// levels coloured per rank, mg_gs_interior: tests/host_solve_mg_gs_dist_shim.cpp, tests/host_solve_mg_gs_dist_main.cpp).  The multicolour
// block ILU(0) has its private layout and the factor step of a node among the host+device functions (ilu_value_offset, ilu_find,
// ilu_factor_node) and its lists and placement among the host ones (ilu_build, ilu_place; tests/host_solve_ilu_shim.cpp); on a
// pattern with ghost columns the same functions factor the owned square (tests/host_solve_ilu_dist_shim.cpp).  The fp32 copy of
// the factor has a layout of its own beside them (ilu_f32_offset, ilu_f32_offsets, ilu_place_f32; tests/host_solve_ilu_f32_shim.cpp).
// Restarted GMRES: the Givens step, the back substitution and the layout of its state (gmres_givens_step, gmres_back_substitute,
// gmres_carve; tests/host_solve_gmres_shim.cpp, tests/host_solve_gmres_main.cpp; the partitioned form of the state, with ghosted basis
// slots and the buffer of the wide all-reduce: tests/host_solve_gmres_dist_shim.cpp, tests/host_solve_gmres_dist_main.cpp).
//
// Pattern (HostPrep::bptr / bcol): node n owns the blocks [bptr[n], bptr[n+1]); block k of the node couples it to
// node bcol[bptr[n] + k] (ascending in k).  The nvar rows of a node share that list, and the values of the node lie
// contiguously as [var a][block k][var b]: scalar CSR on the outside (row n*nvar + a has len*nvar entries whose
// columns are bcol*nvar + b), a block pattern inside -- 4 bytes of index per nvar x nvar block.
#ifndef RDC_SOLVE_H
#define RDC_SOLVE_H
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RDC_SOLVE_HD __host__ __device__ __forceinline__
#else
#define RDC_SOLVE_HD inline
#endif

namespace rdc {

// position in the CSR value array of entry (row node `node`, equation a, block k of the node, unknown b)
RDC_SOLVE_HD int64_t csr_value_offset(const int64_t* bptr, int nvar, int64_t node, int a, int64_t k, int b) {
  const int64_t b0 = bptr[node], len = bptr[node + 1] - b0;
  return (int64_t)nvar * nvar * b0 + ((int64_t)a * len + k) * nvar + b;
}

// scalar column of that entry
RDC_SOLVE_HD int64_t csr_value_column(const int64_t* bptr, const int32_t* bcol, int nvar, int64_t node, int64_t k, int b) {
  return (int64_t)bcol[bptr[node] + k] * nvar + b;
}

// block of node `node` that couples it to itself (binary search, bcol ascends within a node); -1 if the pattern has none
RDC_SOLVE_HD int64_t csr_diag_block(const int64_t* bptr, const int32_t* bcol, int64_t node) {
  int64_t lo = bptr[node], hi = bptr[node + 1] - 1;
  const int64_t b0 = lo;
  while (lo <= hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int64_t c = bcol[mid];
    if (c == node) return mid - b0;
    if (c < node) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

// false for NaN and +-inf; on the bit pattern, so that no floating-point optimisation can change its meaning
RDC_SOLVE_HD bool solve_finite(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, sizeof(u));
  return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// In-place inverse of an NV x NV block (row-major), Gauss-Jordan with partial pivoting.  Every index below is a
// compile-time constant after unrolling (the row exchange is a chain of conditional swaps), so a kernel keeps the block in
// registers.  Returns false -- and leaves `m` unspecified -- for a block that is singular to working precision
// (a zero pivot column) or holds a non-finite entry; the caller must not use the result then.
template <int NV>
RDC_SOLVE_HD bool block_inverse(double (&m)[NV][NV]) {
  double inv[NV][NV];
#pragma unroll
  for (int i = 0; i < NV; i++)
#pragma unroll
    for (int j = 0; j < NV; j++) inv[i][j] = i == j ? 1.0 : 0.0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < NV; c++) {
    // pivot: the first row of c .. NV-1 with the largest |m[r][c]|
    int p = c;
    double best = fabs(m[c][c]);
#pragma unroll
    for (int r = c + 1; r < NV; r++) {
      const double v = fabs(m[r][c]);
      if (v > best) { best = v; p = r; }
    }
#pragma unroll
    for (int r = c + 1; r < NV; r++) {
      if (p == r) {
#pragma unroll
        for (int j = 0; j < NV; j++) {
          double t = m[c][j]; m[c][j] = m[r][j]; m[r][j] = t;
          t = inv[c][j]; inv[c][j] = inv[r][j]; inv[r][j] = t;
        }
      }
    }
    const double piv = m[c][c];
    if (!(fabs(piv) > 0.0) || !solve_finite(piv)) ok = false;   // NaN compares false: reported too
    const double ip = 1.0 / piv;
#pragma unroll
    for (int j = 0; j < NV; j++) { m[c][j] *= ip; inv[c][j] *= ip; }
#pragma unroll
    for (int r = 0; r < NV; r++) {
      if (r == c) continue;
      const double f = m[r][c];
#pragma unroll
      for (int j = 0; j < NV; j++) { m[r][j] -= f * m[c][j]; inv[r][j] -= f * inv[c][j]; }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; i++)
#pragma unroll
    for (int j = 0; j < NV; j++) {
      if (!solve_finite(inv[i][j])) ok = false;
      m[i][j] = inv[i][j];
    }
  return ok;
}

// what the preconditioner stores for one node: precond 2 = inverse of the whole diagonal block, 1 = of its diagonal
// only (point Jacobi), 0 = identity.  `d` holds the diagonal block on entry and D^-1 on exit; false = not invertible
// (d is then the identity, so that an apply stays harmless).
template <int NV>
RDC_SOLVE_HD bool precond_block(double (&d)[NV][NV], int precond) {
  bool ok = true;
  if (precond == 2) {
    ok = block_inverse<NV>(d);
  } else if (precond == 1) {
#pragma unroll
    for (int i = 0; i < NV; i++) {
      const double x = d[i][i];
      if (!(fabs(x) > 0.0) || !solve_finite(x)) ok = false;
#pragma unroll
      for (int j = 0; j < NV; j++) d[i][j] = i == j ? 1.0 / x : 0.0;
    }
  }
  if (precond == 0 || !ok) {
#pragma unroll
    for (int i = 0; i < NV; i++)
#pragma unroll
      for (int j = 0; j < NV; j++) d[i][j] = i == j ? 1.0 : 0.0;
  }
  return ok;
}

// false for NaN and +-inf, as solve_finite
RDC_SOLVE_HD bool solve_finite_f32(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, sizeof(u));
  return (u & 0x7f800000u) != 0x7f800000u;
}

// out = fl32(dinv * a): one block of the fp32 copy of D^-1 A that the mixed-precision iteration streams.  Every product
// sum is accumulated in fp64 in ascending index order (separate multiply and add) and rounded to fp32 once.  Returns
// false if an entry of `out` is not finite: the product overflows fp32 (|.| > 3.4e38) or an input is NaN / inf; the
// caller must not iterate on such a copy.  An entry below the fp32 normal range becomes a subnormal or 0: harmless.
template <int NV>
RDC_SOLVE_HD bool scaled_block_f32(const double (&dinv)[NV][NV], const double (&a)[NV][NV], float (&out)[NV][NV]) {
#if defined(__clang__)
#pragma clang fp contract(off)   // the kernel rounds each product, as the CPU build of the tests does
#endif
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NV; i++)
#pragma unroll
    for (int j = 0; j < NV; j++) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NV; q++) s = s + dinv[i][q] * a[q][j];
      out[i][j] = (float)s;
      if (!solve_finite_f32(out[i][j])) ok = false;
    }
  return ok;
}

// Layout of the fp32 copy (private to rdc_solve.hip): the values of node n start at float offset voff[n] and lie as
// [var a][block k][var b] like the fp64 values, but every one of the nvar rows is padded with zeros to a multiple of
// 4 floats, so that each row starts 16-byte aligned whatever nvar and the row length are (nvar = 5 puts the fp64 rows
// at odd offsets).  voff[n + 1] - voff[n] = nvar * f32_row_stride(nvar, blocks of n).
RDC_SOLVE_HD int64_t f32_row_stride(int nvar, int64_t blocks) { return ((int64_t)nvar * blocks + 3) & ~(int64_t)3; }

// ---- aggregation multigrid (precond 3).  The fixed numbers of the method, all in one place: ----
constexpr int MG_AGG_CAP = 8;           // nodes of an aggregate built in pass 1 (root + 7 neighbours)
constexpr int MG_MIN_FREE = 3;          // free neighbours a free node needs to become a root
constexpr int MG_COARSEST_NODES = 40;   // no further level below a level of at most this many nodes
constexpr int MG_MAX_LEVELS = 10;       // levels, the matrix itself (level 0) included
constexpr int MG_COARSEST_SWEEPS = 8;   // damped block-Jacobi sweeps that stand for the solve on the last level
constexpr int MG_OMEGA_PERMILLE = 600;  // default damping of the smoother, in thousandths (option "mg_omega")
// Gauss-Seidel smoother (option "mg_smoother" = 1): a level of at most this many nodes runs a whole sweep -- on the last level all
// its sweeps -- in one launch of one workgroup (option "mg_gs_fuse" = 0: one launch per colour on every level).
// Measured at K(119) on an MI355X: 54 launches per cycle against 94, and 233.7 / 155.9 ms per solve (first / fifth
// step, FP64) against 233.9 / 156.0 ms -- worth 0.1 to 0.4 ms of a solve, inside the spread of two runs; kept, since it costs nothing.
constexpr int MG_GS_FUSED_NODES = 512;

// out = dinv * a in FP64: the summand of the level-1 Galerkin sum.  Every sum in ascending index order from 0.0, separate
// multiply and add (scaled_block_f32 without its rounding).  scaled_entry is one entry: row `drow` of dinv, column `acol` of a.
template <int NV>
RDC_SOLVE_HD double scaled_entry(const double (&drow)[NV], const double (&acol)[NV]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < NV; q++) s = s + drow[q] * acol[q];
  return s;
}

template <int NV>
RDC_SOLVE_HD void scaled_block(const double (&dinv)[NV][NV], const double (&a)[NV][NV], double (&out)[NV][NV]) {
#pragma unroll
  for (int i = 0; i < NV; i++)
#pragma unroll
    for (int j = 0; j < NV; j++) {
      double col[NV];
#pragma unroll
      for (int q = 0; q < NV; q++) col[q] = a[q][j];
      out[i][j] = scaled_entry<NV>(dinv[i], col);
    }
}

// ---- multicolour block ILU(0) (precond 4): the factor's private layout and the factor step of one node ----
//
// The factor of A^ = D^-1 A lives in a copy of the node-block values, 8 bytes per non-zero, whose layout is private to the library and
// stated here once.  Node i keeps its blocks [bptr[i], bptr[i + 1]) of the pattern, but in ELIMINATION order, (colour, node id)
// ascending: position p of the node couples it to node pcol[bptr[i] + p]; the first nlow[i] positions are the lower blocks (a
// column of a lower colour: L_ip, the identity on L's diagonal is not stored), position nlow[i] is the diagonal block (U_ii), the
// rest are the upper blocks (U_ip).  The values of a node lie as three runs, each [var a][block][var b] like the CSR values:
//   lower  nvar x (nlow * nvar)   at nvar^2 * bptr[i]                      what the forward sweep reads, contiguous
//   diag   nvar x nvar            behind it                                (the sweeps read U_ii^-1 from an array of its own)
//   upper  nvar x (nup * nvar)    behind that, nup = len - nlow - 1        what the backward sweep reads, contiguous
// so that forward and backward together cross the factor once: 8 nnz + 4 blocks bytes.
// On a pattern with ghost columns (precond 5, the rank-local factor: the ILU(0) of the OWNED SQUARE, rows and columns below
// n_owned) the ghost columns of a node stand last in its private row, in ascending id, behind its nown[i] owned positions, and
// nothing else changes: elimination order, nlow and the three runs are those of the nown[i] owned positions, nup = nown - nlow - 1.
// The node keeps its nvar^2 * len values at nvar^2 * bptr[i]; the nvar^2 * (len - nown) behind the upper run are the slots of the
// ghost blocks, which nothing writes or reads.  No node has a ghost column: nown is not kept, and everything is as stated above.
// b0 = bptr[i], len = the positions the runs cover: bptr[i + 1] - b0, or nown[i] on a pattern with ghost columns; nl = nlow[i]
RDC_SOLVE_HD int64_t ilu_value_offset(int64_t b0, int nvar, int64_t len, int64_t nl, int a, int64_t p, int b) {
  const int64_t base = (int64_t)nvar * nvar * b0;
  if (p < nl) return base + ((int64_t)a * nl + p) * nvar + b;
  if (p == nl) return base + (int64_t)nvar * nvar * nl + (int64_t)a * nvar + b;
  return base + (int64_t)nvar * nvar * (nl + 1) + ((int64_t)a * (len - nl - 1) + (p - nl - 1)) * nvar + b;
}

// The fp32 copy of the factor (option "ilu_factor_bits" = 32; DESIGN.md 7.4, "fp32 factor"): what the sweeps stream instead of the
// FP64 runs above.  It is rounded from them after the factorisation and has a layout and offsets of its own: node i starts at
// float offset foff[i] and keeps its lower run and, behind it, its upper run, each [var a][block][var b] as above, with every one
// of the nvar rows of a run padded with zeros to a multiple of 4 floats (f32_row_stride: a row starts 16-byte aligned).  There is
// no diagonal block (the sweeps read the FP64 U_ii^-1), and on lists with ghost columns the upper run ends at the owned positions:
// a ghost block has no slot at all.  len and nl as for ilu_value_offset; p != nl.
RDC_SOLVE_HD int64_t ilu_f32_node_floats(int nvar, int64_t len, int64_t nl) {
  return (int64_t)nvar * (f32_row_stride(nvar, nl) + f32_row_stride(nvar, len - nl - 1));
}
RDC_SOLVE_HD int64_t ilu_f32_offset(int64_t f0, int nvar, int64_t len, int64_t nl, int a, int64_t p, int b) {
  if (p < nl) return f0 + (int64_t)a * f32_row_stride(nvar, nl) + p * nvar + b;
  return f0 + (int64_t)nvar * f32_row_stride(nvar, nl) + (int64_t)a * f32_row_stride(nvar, len - nl - 1) + (p - nl - 1) * nvar + b;
}

// position of column node j in the private row `row` (len entries, ascending in (colour, node id); with ghost columns: the owned
// positions only, since `colour` has no entry for a ghost); -1 if the row has none
RDC_SOLVE_HD int64_t ilu_find(const int32_t* row, int64_t len, const int32_t* colour, int32_t j) {
  const int32_t cj = colour[j];
  int64_t lo = 0, hi = len - 1;
  while (lo <= hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int32_t m = row[mid], cm = colour[m];
    if (m == j) return mid;
    if (cm < cj || (cm == cj && m < j)) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

// The factor of node i, all of whose row neighbours of a lower colour are factored: for its lower positions p in order (node
// k = pcol[p]) L_ip = F_ip U_kk^-1, then F_ij -= L_ip U_kj for every upper block j of row k that row i has as well (at a position
// behind p); at the end U_ii^-1 (block_inverse).  `lanes` callers share the node: each computes L_ip for itself, lane 0 stores it,
// and the upper blocks of row k are dealt out lane, lane + lanes, ... -- their targets in row i are distinct.  sync(): what makes
// the stores of all lanes visible to all lanes before the next position is read (one lane: nothing).  Every sum is a chain of fma
// in ascending index order, the updates of a block come in the order of p: no atomics, the same bits whatever `lanes` is.
// Returns (lane 0; the others true) whether U_ii could be inverted; if not, uinv of the node is the identity.
// OWNED (a pattern with ghost columns): the rows end at their owned positions, nown[i] and nown[k]; no ghost block is touched.
template <int NV, bool OWNED = false, class Sync>
RDC_SOLVE_HD bool ilu_factor_node(const int64_t* bptr, const int32_t* pcol, const int32_t* nlow, const int32_t* colour,
                                  double* val, double* uinv, int64_t i, int lane, int lanes, Sync&& sync, const int32_t* nown = nullptr) {
  const int64_t b0 = bptr[i], len = OWNED ? (int64_t)nown[i] : bptr[i + 1] - b0, nl = nlow[i];
  for (int64_t p = 0; p < nl; p++) {
    const int64_t k = pcol[b0 + p];
    double l[NV][NV];
    {
      double f[NV][NV];
#pragma unroll
      for (int a = 0; a < NV; a++)
#pragma unroll
        for (int b = 0; b < NV; b++) f[a][b] = val[ilu_value_offset(b0, NV, len, nl, a, p, b)];
#pragma unroll
      for (int a = 0; a < NV; a++)
#pragma unroll
        for (int b = 0; b < NV; b++) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < NV; q++) s = fma(f[a][q], uinv[(k * NV + q) * NV + b], s);
          l[a][b] = s;
        }
    }
    if (lane == 0)
#pragma unroll
      for (int a = 0; a < NV; a++)
#pragma unroll
        for (int b = 0; b < NV; b++) val[ilu_value_offset(b0, NV, len, nl, a, p, b)] = l[a][b];
    const int64_t k0 = bptr[k], klen = OWNED ? (int64_t)nown[k] : bptr[k + 1] - k0, knl = nlow[k];
    for (int64_t q = knl + 1 + lane; q < klen; q += lanes) {
      const int64_t at = ilu_find(pcol + b0, len, colour, pcol[k0 + q]);
      if (at < 0) continue;
      double u[NV][NV];
#pragma unroll
      for (int a = 0; a < NV; a++)
#pragma unroll
        for (int b = 0; b < NV; b++) u[a][b] = val[ilu_value_offset(k0, NV, klen, knl, a, q, b)];
#pragma unroll
      for (int a = 0; a < NV; a++)
#pragma unroll
        for (int b = 0; b < NV; b++) {
          const int64_t o = ilu_value_offset(b0, NV, len, nl, a, at, b);
          double t = val[o];
#pragma unroll
          for (int c = 0; c < NV; c++) t = fma(-l[a][c], u[c][b], t);
          val[o] = t;
        }
    }
    sync();
  }
  bool ok = true;
  if (lane == 0) {
    double d[NV][NV];
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) d[a][b] = val[ilu_value_offset(b0, NV, len, nl, a, nl, b)];
    ok = precond_block<NV>(d, 2);
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) uinv[(i * NV + a) * NV + b] = d[a][b];
  }
  return ok;
}

}  // namespace rdc

#include <algorithm>
#include <utility>
#include <vector>
namespace rdc {

// Aggregates of the node-block graph (n nodes, pattern bptr / bcol, no ghost columns); deterministic, ascending node order.
// Pass 1: a free node with at least MG_MIN_FREE free neighbours becomes a root and takes the first MG_AGG_CAP - 1 of them.
// Pass 2: a node still free joins the aggregate of its first neighbour that has one by then (nodes joined earlier in this
// pass included), or becomes a singleton.  agg[n] = aggregate of node n; returns their number, *n_pass1 = those of pass 1.
inline int64_t mg_aggregate(int64_t n, const int64_t* bptr, const int32_t* bcol, int32_t* agg, int64_t* n_pass1) {
  for (int64_t i = 0; i < n; i++) agg[i] = -1;
  int64_t na = 0;
  for (int64_t i = 0; i < n; i++) {
    if (agg[i] >= 0) continue;
    int nfree = 0;
    for (int64_t k = bptr[i]; k < bptr[i + 1] && nfree < MG_MIN_FREE; k++) nfree += bcol[k] != i && agg[bcol[k]] < 0;
    if (nfree < MG_MIN_FREE) continue;
    agg[i] = (int32_t)na;
    int taken = 0;
    for (int64_t k = bptr[i]; k < bptr[i + 1] && taken < MG_AGG_CAP - 1; k++)
      if (bcol[k] != i && agg[bcol[k]] < 0) { agg[bcol[k]] = (int32_t)na; taken++; }
    na++;
  }
  if (n_pass1) *n_pass1 = na;
  for (int64_t i = 0; i < n; i++) {
    if (agg[i] >= 0) continue;
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++)
      if (bcol[k] != i && agg[bcol[k]] >= 0) { agg[i] = agg[bcol[k]]; break; }
    if (agg[i] < 0) agg[i] = (int32_t)na++;
  }
  return na;
}

// One coarsening step: what takes level l (n_fine nodes) to level l + 1 (n nodes), all lists in ascending order.
struct MgLevelHost {
  int64_t n_fine = 0, n = 0, n_pass1 = 0;
  std::vector<int32_t> agg;      // [n_fine] aggregate of a fine node: prolongation
  std::vector<int64_t> mptr;     // [n + 1]  members of aggregate I: member[mptr[I] .. mptr[I + 1]): restriction
  std::vector<int32_t> member;   // [n_fine]
  std::vector<int64_t> bptr;     // [n + 1]  node-block pattern of the coarse matrix (bcol ascends within a node)
  std::vector<int32_t> bcol;
  std::vector<int32_t> brow;     // [coarse blocks] node of a coarse block
  std::vector<int64_t> cptr;     // [coarse blocks + 1] fine blocks that sum into coarse block c: cidx[cptr[c] .. cptr[c + 1]),
  std::vector<int32_t> cidx;     // [fine blocks] ... ascending = sorted by (fine node, k); cidx = bptr_fine[node] + k
  std::vector<int32_t> cnode;    // [fine blocks] ... and the fine node of each (the value layout needs the node's row length)
};

// The lists of a coarsening step from its aggregates: L.n_fine, L.n and L.agg are given, and L.agg has an entry for every column
// of the pattern (behind the n_fine rows: the coarse number of a ghost column, mg_halo_coarsen).  Rows, members and
// contributions are those of the n_fine row nodes only.  false: the coarse level would have 2^31 blocks or more
inline bool mg_coarsen_lists(const int64_t* bptr, const int32_t* bcol, MgLevelHost& L) {
  const int64_t n_fine = L.n_fine, na = L.n, nblk = bptr[n_fine];
  L.mptr.assign((size_t)na + 1, 0);
  for (int64_t i = 0; i < n_fine; i++) L.mptr[(size_t)L.agg[i] + 1]++;
  for (int64_t I = 0; I < na; I++) L.mptr[(size_t)I + 1] += L.mptr[(size_t)I];
  L.member.resize((size_t)n_fine);
  {
    std::vector<int64_t> fill(L.mptr.begin(), L.mptr.end() - 1);
    for (int64_t i = 0; i < n_fine; i++) L.member[(size_t)fill[(size_t)L.agg[i]]++] = (int32_t)i;
  }
  // coarse rows: the distinct aggregates of the columns of the members' blocks
  L.bptr.assign((size_t)na + 1, 0);
  std::vector<int32_t> row;
  for (int64_t I = 0; I < na; I++) {
    row.clear();
    for (int64_t m = L.mptr[(size_t)I]; m < L.mptr[(size_t)I + 1]; m++)
      for (int64_t k = bptr[L.member[(size_t)m]]; k < bptr[L.member[(size_t)m] + 1]; k++) row.push_back(L.agg[(size_t)bcol[k]]);
    std::sort(row.begin(), row.end());
    row.erase(std::unique(row.begin(), row.end()), row.end());
    L.bcol.insert(L.bcol.end(), row.begin(), row.end());
    L.brow.resize(L.bcol.size(), (int32_t)I);
    L.bptr[(size_t)I + 1] = (int64_t)L.bcol.size();
    if (L.bcol.size() >= ((size_t)1 << 31)) return false;
  }
  // coarse block of every fine block, then the lists by a counting sort (stable: ascending fine block within a coarse one)
  const int64_t ncb = (int64_t)L.bcol.size();
  std::vector<int32_t> cmap((size_t)nblk);
  L.cptr.assign((size_t)ncb + 1, 0);
  for (int64_t i = 0; i < n_fine; i++) {
    const int64_t I = L.agg[(size_t)i];
    const int32_t* r0 = L.bcol.data() + L.bptr[(size_t)I];
    const int32_t* r1 = L.bcol.data() + L.bptr[(size_t)I + 1];
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++) {
      const int64_t c = L.bptr[(size_t)I] + (std::lower_bound(r0, r1, L.agg[(size_t)bcol[k]]) - r0);
      cmap[(size_t)k] = (int32_t)c;
      L.cptr[(size_t)c + 1]++;
    }
  }
  for (int64_t c = 0; c < ncb; c++) L.cptr[(size_t)c + 1] += L.cptr[(size_t)c];
  L.cidx.resize((size_t)nblk);
  L.cnode.resize((size_t)nblk);
  std::vector<int64_t> fill(L.cptr.begin(), L.cptr.end() - 1);
  for (int64_t i = 0; i < n_fine; i++)
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++) {
      const int64_t at = fill[(size_t)cmap[(size_t)k]]++;
      L.cidx[(size_t)at] = (int32_t)k;
      L.cnode[(size_t)at] = (int32_t)i;
    }
  return true;
}

// false: as mg_coarsen_lists
inline bool mg_coarsen(int64_t n_fine, const int64_t* bptr, const int32_t* bcol, MgLevelHost& L) {
  L = MgLevelHost();
  L.n_fine = n_fine;
  L.agg.resize((size_t)n_fine);
  L.n = mg_aggregate(n_fine, bptr, bcol, L.agg.data(), &L.n_pass1);
  return mg_coarsen_lists(bptr, bcol, L);
}

// The whole hierarchy below a matrix of n nodes: steps[l] takes level l to level l + 1.  Stops at a level of at most
// MG_COARSEST_NODES nodes, at MG_MAX_LEVELS levels, or when a coarsening would merge nothing.  false: as mg_coarsen.
inline bool mg_build(int64_t n, const int64_t* bptr, const int32_t* bcol, std::vector<MgLevelHost>& steps) {
  steps.clear();
  if (bptr[n] >= ((int64_t)1 << 31)) return false;
  while (n > MG_COARSEST_NODES && (int)steps.size() + 1 < MG_MAX_LEVELS) {
    MgLevelHost L;
    if (!mg_coarsen(n, bptr, bcol, L)) return false;
    if (L.n >= n) break;
    steps.push_back(std::move(L));
    n = steps.back().n;
    bptr = steps.back().bptr.data();
    bcol = steps.back().bcol.data();
  }
  return true;
}

// ---- the hierarchy on a ghosted context (rdc_solve_dist_mg).  Aggregates never cross a partition, so a rank owns
// whole coarse rows and builds them alone; what every level needs is its ghost layer.  The steps below are what one rank does
// between the two collective calls of a coarsening step (an all-reduce that decides, an exchange of aggregate numbers); the caller
// supplies those, so that a CPU build can drive several ranks in one process (tests/host_solve_mg_dist_shim.cpp). ----

// The ghost layer of one level of one rank.  Peers in the caller's order; the send list and the ghost tail are both grouped by
// peer in that order, and the send segment for peer q names this rank's nodes in the order of q's ghost segment from this rank.
struct MgHalo {
  int64_t n_owned = 0, n_ghost = 0;
  std::vector<int64_t> send_off, ghost_off;   // [peers + 1] segment bounds, in nodes
  std::vector<int32_t> send_nodes;            // [send_off.back()] owned nodes, send order
  std::vector<int64_t> send_ptr;              // [n_owned + 1] the slots of the send buffer that hold node n: send_slot[send_ptr[n] ..
  std::vector<int32_t> send_slot;             // [send_off.back()] ... send_ptr[n + 1]), ascending (a node has one per peer that sees it)
  int64_t n_send() const { return (int64_t)send_nodes.size(); }
  int peers() const { return (int)send_off.size() - 1; }
};

// send_ptr / send_slot from send_nodes (counting sort: the slots of a node ascend)
inline void mg_halo_slots(MgHalo& H) {
  H.send_ptr.assign((size_t)H.n_owned + 1, 0);
  for (int32_t n : H.send_nodes) H.send_ptr[(size_t)n + 1]++;
  for (int64_t n = 0; n < H.n_owned; n++) H.send_ptr[(size_t)n + 1] += H.send_ptr[(size_t)n];
  H.send_slot.resize(H.send_nodes.size());
  std::vector<int64_t> fill(H.send_ptr.begin(), H.send_ptr.end() - 1);
  for (size_t i = 0; i < H.send_nodes.size(); i++) H.send_slot[(size_t)fill[(size_t)H.send_nodes[i]]++] = (int32_t)i;
}

// Level 0 from the plan (send list) and the per-peer counts.  0 = fine; 1 = a count is negative; 2 = the send counts do not add up to
// the send list; 3 = the ghost counts do not add up to the ghost tail; 4 = a send id is not an owned node
inline int mg_halo_plan(int64_t n_owned, int64_t n_ghost, int64_t n_send, const int32_t* send_nodes, int n_peers,
                        const int64_t* send_count, const int64_t* ghost_count, MgHalo& H) {
  H = MgHalo();
  H.n_owned = n_owned; H.n_ghost = n_ghost;
  H.send_off.assign((size_t)n_peers + 1, 0); H.ghost_off.assign((size_t)n_peers + 1, 0);
  for (int q = 0; q < n_peers; q++) {
    if (send_count[q] < 0 || ghost_count[q] < 0) return 1;
    H.send_off[(size_t)q + 1] = H.send_off[(size_t)q] + send_count[q];
    H.ghost_off[(size_t)q + 1] = H.ghost_off[(size_t)q] + ghost_count[q];
  }
  if (H.send_off.back() != n_send) return 2;
  if (H.ghost_off.back() != n_ghost) return 3;
  for (int64_t i = 0; i < n_send; i++)
    if (send_nodes[i] < 0 || send_nodes[i] >= n_owned) return 4;
  H.send_nodes.assign(send_nodes, send_nodes + n_send);
  mg_halo_slots(H);
  return 0;
}

// Step 1 of a coarsening: mg_aggregate on the edges whose two ends this rank owns (ghost columns ignored; the same passes, constants
// and ascending order).  Sizes L.agg for every column and fills its owned part; a rank that can merge nothing gets the identity.
// ids_out [F.n_send()]: what the exchange of width 1 sends, the aggregate of every send node as a double (exact below 2^53).
inline void mg_dist_aggregate(const MgHalo& F, const int64_t* bptr, const int32_t* bcol, MgLevelHost& L, double* ids_out) {
  const int64_t n = F.n_owned;
  std::vector<int64_t> optr((size_t)n + 1, 0);
  std::vector<int32_t> ocol;
  for (int64_t i = 0; i < n; i++) {
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++)
      if (bcol[k] < n) ocol.push_back(bcol[k]);
    optr[(size_t)i + 1] = (int64_t)ocol.size();
  }
  L = MgLevelHost();
  L.n_fine = n;
  L.agg.assign((size_t)(n + F.n_ghost), -1);
  L.n = mg_aggregate(n, optr.data(), ocol.data(), L.agg.data(), &L.n_pass1);
  for (int64_t i = 0; i < F.n_send(); i++) ids_out[i] = (double)L.agg[(size_t)F.send_nodes[(size_t)i]];
}

// Step 2, behind the exchange: ids_in [F.n_ghost] = the owner's aggregate number of every ghost node.  The coarse ghosts from peer q
// are the distinct ids of q's ghost segment in order of first appearance, numbered behind the owned aggregates in peer order; the
// coarse send segment for q is the distinct own aggregates of the fine send segment for q, in order of first appearance.  The two
// sequences are the same list on the two sides, so the coarse level needs no message of its own.  Fills the ghost part of L.agg,
// the lists of L and the coarse ghost layer C.  false: an id is not a count below 2^31, or as mg_coarsen_lists.
inline bool mg_dist_coarsen(const MgHalo& F, const int64_t* bptr, const int32_t* bcol, const double* ids_in, MgLevelHost& L, MgHalo& C) {
  const int peers = F.peers();
  C = MgHalo();
  C.n_owned = L.n;
  C.send_off.assign((size_t)peers + 1, 0); C.ghost_off.assign((size_t)peers + 1, 0);
  std::vector<std::pair<int64_t, int32_t>> known;   // (id, coarse number) of the segment at hand, sorted by id
  int64_t next = L.n;
  for (int q = 0; q < peers; q++) {
    known.clear();
    for (int64_t g = F.ghost_off[(size_t)q]; g < F.ghost_off[(size_t)q + 1]; g++) {
      const double idd = ids_in[g];
      if (!(idd >= 0.0) || !(idd < 2147483648.0) || idd != (double)(int64_t)idd) return false;
      const int64_t id = (int64_t)idd;
      auto at = std::lower_bound(known.begin(), known.end(), std::make_pair(id, (int32_t)-1));
      if (at == known.end() || at->first != id) {
        if (next >= ((int64_t)1 << 31) - 1) return false;
        at = known.insert(at, std::make_pair(id, (int32_t)next++));
      }
      L.agg[(size_t)(F.n_owned + g)] = at->second;
    }
    C.ghost_off[(size_t)q + 1] = next - L.n;
    known.clear();
    for (int64_t i = F.send_off[(size_t)q]; i < F.send_off[(size_t)q + 1]; i++) {
      const int64_t id = L.agg[(size_t)F.send_nodes[(size_t)i]];
      auto at = std::lower_bound(known.begin(), known.end(), std::make_pair(id, (int32_t)-1));
      if (at == known.end() || at->first != id) {
        known.insert(at, std::make_pair(id, (int32_t)0));
        C.send_nodes.push_back((int32_t)id);
      }
    }
    C.send_off[(size_t)q + 1] = (int64_t)C.send_nodes.size();
  }
  C.n_ghost = next - L.n;
  mg_halo_slots(C);
  return mg_coarsen_lists(bptr, bcol, L);
}

// The collective stopping rule, on the two sums every rank holds after the all-reduce of a step: the nodes of the level at hand over
// all ranks, and the number of ranks whose aggregation merged something.  `levels` exist so far, the matrix included.  With one
// rank this is the rule of mg_build.
inline bool mg_dist_goes_on(int levels, double global_nodes, double ranks_that_merged) {
  return global_nodes > (double)MG_COARSEST_NODES && levels < MG_MAX_LEVELS && ranks_that_merged > 0.0;
}

// One level of the multigrid hierarchy on the device.  Level 0 is the matrix itself (bptr / bcol only: its values are the
// context's, its D^-1 the solver's).  A level l >= 1 owns a matrix in the node-block layout, its D_l^-1, three vectors, and
// the lists that take level l - 1 to it (MgLevelHost of that step).
struct MgLevelDev {
  int64_t n = 0, blocks = 0;
  const int64_t* bptr = nullptr;
  const int32_t* bcol = nullptr;
  double *val = nullptr, *dinv = nullptr, *x = nullptr, *r = nullptr, *t = nullptr;
  const int32_t *agg = nullptr, *member = nullptr, *brow = nullptr, *cidx = nullptr, *cnode = nullptr;
  const int64_t *mptr = nullptr, *cptr = nullptr;
  // across ranks (level >= 1): x has a ghost tail of n_ghost nodes behind its n owned ones; `send` (n_send nodes) is filled by the
  // kernel that last writes x, through the slots of every node (MgHalo::send_ptr / send_slot).  send_off / ghost_off: HOST arrays
  // of peers + 1 offsets in doubles, what the sized exchange callback gets.
  int64_t n_ghost = 0, n_send = 0;
  double* send = nullptr;
  const int64_t* send_ptr = nullptr;
  const int32_t* send_slot = nullptr;
  const int64_t *send_off = nullptr, *ghost_off = nullptr;
};

struct MgDev {
  int n_levels = 0;                      // level 0 included
  MgLevelDev lv[MG_MAX_LEVELS];
  double *ph = nullptr, *sh = nullptr;   // M p and M s of the right-preconditioned iteration (n_owned * nvar each)
  double* t0 = nullptr;                  // A^ x of the level-0 smoother
  double omega = 0.0;
  float setup_ms = 0.0f;                 // out: device time of the Galerkin products and the D_l^-1 of the last solve
};

// The two device arenas of a hierarchy, stated once: `idx` holds every list of every step, `val` the vectors of the iteration and
// every matrix / D_l^-1 / vector of the levels; each array starts MG_ALIGN-aligned.  mg_place walks the levels once and fills `g`.
// Arenas without a base measure: `used` ends at the bytes to allocate and every pointer of `g` stays null.  With a base (of at
// least the measured bytes) they place: `g` points into them, and upload(at, source, bytes) is called for every list that is not empty.
constexpr size_t MG_ALIGN = 256;

struct MgArena {
  char* base = nullptr;
  size_t used = 0;
  void* take(size_t bytes) {
    void* at = base ? base + used : nullptr;
    used += (bytes + MG_ALIGN - 1) & ~(MG_ALIGN - 1);
    return at;
  }
};

// halos (across ranks only): halos[l] is the ghost layer of level l, level 0 = the plan.  M p and M s then get the ghost tail the
// outer operator receives into, and every level below its tail of x, its send buffer and its slot lists; without halos the
// layout is that of rdc_solve, byte for byte.
template <class Upload>
inline void mg_place(const std::vector<MgLevelHost>& steps, int nvar, int64_t n_owned, int64_t blocks, MgArena& idx, MgArena& val,
                     MgDev& g, Upload&& upload, const std::vector<MgHalo>* halos = nullptr) {
  auto list = [&](const auto& v) {
    const size_t bytes = v.size() * sizeof(v[0]);
    void* at = idx.take(bytes);
    if (at && bytes) upload(at, (const void*)v.data(), bytes);
    return (decltype(v.data()))at;
  };
  auto vec = [&](int64_t doubles) { return (double*)val.take((size_t)doubles * sizeof(double)); };
  g = MgDev();
  g.n_levels = (int)steps.size() + 1;
  g.lv[0].n = n_owned; g.lv[0].blocks = blocks;
  const int64_t n0 = std::max<int64_t>(n_owned * nvar, 1);
  const int64_t n0g = halos ? std::max<int64_t>((n_owned + (*halos)[0].n_ghost) * nvar, 1) : n0;
  g.lv[0].n_ghost = halos ? (*halos)[0].n_ghost : 0;
  g.ph = vec(n0g); g.sh = vec(n0g); g.t0 = vec(n0);
  for (size_t l = 0; l < steps.size(); l++) {
    const MgLevelHost& L = steps[l];
    MgLevelDev& D = g.lv[l + 1];
    D.n = L.n; D.blocks = (int64_t)L.bcol.size();
    D.agg = list(L.agg); D.mptr = list(L.mptr); D.member = list(L.member);
    D.bptr = list(L.bptr); D.bcol = list(L.bcol); D.brow = list(L.brow);
    D.cptr = list(L.cptr); D.cidx = list(L.cidx); D.cnode = list(L.cnode);
    D.val = vec(D.blocks * nvar * nvar); D.dinv = vec(L.n * nvar * nvar);
    if (halos) {
      const MgHalo& H = (*halos)[l + 1];
      D.n_ghost = H.n_ghost; D.n_send = H.n_send();
      D.send_ptr = list(H.send_ptr); D.send_slot = list(H.send_slot);
      D.send = vec(std::max<int64_t>(D.n_send * nvar, 1));
    }
    D.x = vec((L.n + D.n_ghost) * nvar); D.r = vec(L.n * nvar); D.t = vec(L.n * nvar);
  }
}

// ---- multicolour Gauss-Seidel smoother (option "mg_smoother" = 1): the colours of one level ----

// Colour lists of the node-block graph of one level: the nodes of colour c are nodes[cptr[c] .. cptr[c + 1]), ascending.
struct MgColours {
  std::vector<int32_t> colour;   // [n] colour of a node
  std::vector<int64_t> cptr;     // [colours + 1]
  std::vector<int32_t> nodes;    // [n]
  int n_colours() const { return (int)cptr.size() - 1; }
};

// Greedy colouring (n nodes, pattern bptr / bcol): nodes in ascending order, each takes the smallest colour that no row neighbour
// with a colour already holds; self and columns >= n are ignored; no cap on the number of colours.  Then one pass over every block
// (i, j), i != j: false if its two nodes share a colour, which only a structurally asymmetric pattern brings about -- a sweep
// over such lists would race, so the caller must not run one.
inline bool mg_colour(int64_t n, const int64_t* bptr, const int32_t* bcol, MgColours& C) {
  C = MgColours();
  C.colour.assign((size_t)n, -1);
  std::vector<int64_t> held;   // held[c] == i + 1: a neighbour of node i has colour c
  for (int64_t i = 0; i < n; i++) {
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++) {
      const int64_t j = bcol[k];
      if (j != i && j < n && C.colour[(size_t)j] >= 0) held[(size_t)C.colour[(size_t)j]] = i + 1;
    }
    size_t c = 0;
    while (c < held.size() && held[c] == i + 1) c++;
    if (c == held.size()) held.push_back(0);
    C.colour[(size_t)i] = (int32_t)c;
  }
  C.cptr.assign(held.size() + 1, 0);
  for (int64_t i = 0; i < n; i++) C.cptr[(size_t)C.colour[(size_t)i] + 1]++;
  for (size_t c = 0; c < held.size(); c++) C.cptr[c + 1] += C.cptr[c];
  C.nodes.resize((size_t)n);
  std::vector<int64_t> fill(C.cptr.begin(), C.cptr.end() - 1);
  for (int64_t i = 0; i < n; i++) C.nodes[(size_t)fill[(size_t)C.colour[(size_t)i]]++] = (int32_t)i;
  for (int64_t i = 0; i < n; i++)
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++)
      if (bcol[k] != i && bcol[k] < n && C.colour[(size_t)bcol[k]] == C.colour[(size_t)i]) return false;
  return true;
}

// The colour lists of every level on the device: one allocation, measured and placed like the arenas of mg_place (MgArena:
// no base measures).  cptr_host: the same pointer array on the host, what the per-colour launches take their bounds from; it
// points into `cols` and lives as long as they do.
struct MgGsLevel {
  int n_colours = 0;
  const int32_t* nodes = nullptr;
  const int64_t* cptr = nullptr;
  const int64_t* cptr_host = nullptr;
};

struct MgGsDev {
  int n_levels = 0;
  MgGsLevel lv[MG_MAX_LEVELS];
  bool fuse = true;   // option "mg_gs_fuse"
  int64_t int0 = 0;   // partitioned hierarchy: the leading nodes of colour 0 of level 0 that lie below "interior_nodes" (mg_gs_interior)
};

// Nodes are numbered interior first and a colour list ascends, so the interior nodes of colour 0 are a prefix of its list: their count.
inline int64_t mg_gs_interior(const MgColours& C, int64_t n_int) {
  if (C.n_colours() < 1) return 0;
  const auto c0 = C.nodes.begin() + C.cptr[0], c1 = C.nodes.begin() + C.cptr[1];
  return std::lower_bound(c0, c1, n_int, [](int32_t node, int64_t bound) { return (int64_t)node < bound; }) - c0;
}

template <class Upload>
inline void mg_gs_place(const std::vector<MgColours>& cols, MgArena& arena, MgGsDev& g, Upload&& upload) {
  auto list = [&](const auto& v) {
    const size_t bytes = v.size() * sizeof(v[0]);
    void* at = arena.take(bytes);
    if (at && bytes) upload(at, (const void*)v.data(), bytes);
    return (decltype(v.data()))at;
  };
  g = MgGsDev();
  g.n_levels = (int)cols.size();
  for (size_t l = 0; l < cols.size(); l++) {
    g.lv[l].n_colours = cols[l].n_colours();
    g.lv[l].nodes = list(cols[l].nodes);
    g.lv[l].cptr = list(cols[l].cptr);
    g.lv[l].cptr_host = cols[l].cptr.data();
  }
}

// ---- multicolour block ILU(0) (precond 4, and 5: the rank-local factor): the lists of a mesh, and where the factor lies on the device ----

// What the private layout (ilu_value_offset, above) needs beside bptr: the colours of level 0 (mg_colour) and every row in
// elimination order.  Built on the host once per mesh.
struct IluHost {
  MgColours col;
  std::vector<int32_t> pcol;   // [blocks] column node of every position, per node ascending in (colour, node id), ghost columns last
  std::vector<int32_t> nlow;   // [n] lower blocks of a node = position of its diagonal block
  std::vector<int32_t> nown;   // [n] owned positions of a node; EMPTY if no node has a ghost column (they are bptr[i + 1] - bptr[i])
};

// 0 = fine; 1 = the pattern is not structurally symmetric (mg_colour refuses it: a colour would not be independent);
// 2 = node *where has no diagonal block, or a column that is no row (a ghost).
// ghosts: columns >= n are ghost columns and legal (2 then: no diagonal block, or a negative column).  The lists are those of the
// owned square: mg_colour ignores the ghost columns, they stand last in every private row and count into neither nlow nor nown.
inline int ilu_build(int64_t n, const int64_t* bptr, const int32_t* bcol, IluHost& H, int64_t* where, bool ghosts = false) {
  H = IluHost();
  bool any_ghost = false;
  for (int64_t i = 0; i < n; i++) {
    bool diag = false;
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++) {
      if (bcol[k] < 0 || (bcol[k] >= n && !ghosts)) { *where = i; return 2; }
      any_ghost = any_ghost || bcol[k] >= n;
      diag = diag || bcol[k] == i;
    }
    if (!diag) { *where = i; return 2; }
  }
  if (!mg_colour(n, bptr, bcol, H.col)) return 1;
  const std::vector<int32_t>& colour = H.col.colour;
  H.pcol.assign(bcol, bcol + bptr[n]);
  H.nlow.assign((size_t)n, 0);
  if (any_ghost) H.nown.assign((size_t)n, 0);
  for (int64_t i = 0; i < n; i++) {
    std::sort(H.pcol.begin() + bptr[i], H.pcol.begin() + bptr[i + 1], [&](int32_t x, int32_t y) {
      if (x >= n || y >= n) return x < y;   // a ghost behind every owned column, ghosts by id
      return colour[(size_t)x] != colour[(size_t)y] ? colour[(size_t)x] < colour[(size_t)y] : x < y;
    });
    int32_t nl = 0, no = 0;
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++) {
      if (bcol[k] >= n) continue;
      no++;
      nl += colour[(size_t)bcol[k]] < colour[(size_t)i];
    }
    H.nlow[(size_t)i] = nl;
    if (any_ghost) H.nown[(size_t)i] = no;
  }
  return 0;
}

// The factorisation of one whole matrix on the host, node after node in elimination order with one lane (tests, and the yardstick
// of what the per-colour launches compute): val holds A^ in the private layout on entry and the factor on exit, uinv [n][NV][NV]
// the U_ii^-1.  Returns the number of nodes whose U_ii could not be inverted.  On lists with ghost columns: the factor of the owned
// square; the slots of the ghost blocks are neither read nor written.
template <int NV>
inline int64_t ilu_factor_host(int64_t n, const int64_t* bptr, const IluHost& H, double* val, double* uinv) {
  int64_t bad = 0;
  for (int64_t at = 0; at < n; at++) {
    const int64_t i = H.col.nodes[(size_t)at];
    bad += H.nown.empty() ? !ilu_factor_node<NV>(bptr, H.pcol.data(), H.nlow.data(), H.col.colour.data(), val, uinv, i, 0, 1, [] {})
                          : !ilu_factor_node<NV, true>(bptr, H.pcol.data(), H.nlow.data(), H.col.colour.data(), val, uinv, i, 0, 1, [] {}, H.nown.data());
  }
  return bad;
}

// The factor on the device.  Two allocations, measured and placed like the arenas of mg_place (MgArena: no base measures):
// `idx` holds pcol, nlow, the colours and the colour lists, `val` the factor, the U_ii^-1 and the two vectors M p and M s of the
// right-preconditioned iteration.  cptr_host: the bounds of the colour lists on the host (it points into H).
// nown: the owned positions per node, behind the other lists; null on a mesh without ghost columns (IluHost::nown is empty), whose
// two allocations are then byte for byte what they were before ghost columns were taken.  n_nodes (>= n): M p and M s get the ghost
// tail the operator of a partitioned solve receives into.
struct IluDev {
  int n_colours = 0;
  const int32_t *pcol = nullptr, *nlow = nullptr, *colour = nullptr, *nodes = nullptr, *nown = nullptr;
  const int64_t* cptr_host = nullptr;
  double *val = nullptr, *uinv = nullptr, *ph = nullptr, *sh = nullptr;
  float setup_ms = 0.0f;   // out: device time of the copy of A^ and the factorisation (and the rounding) of the last solve
  // the fp32 copy of the factor (ilu_place_f32; a third allocation, made at the first solve with "ilu_factor_bits" = 32)
  const int64_t* foff = nullptr;   // float offset of every node, and the total: n + 1 entries
  float* val32 = nullptr;
  bool want32 = false;             // in: the set-up rounds the factor into val32, and the sweeps stream it unless an entry overflowed
  int bits = 0;                    // out: what the sweeps of the last solve or apply hook streamed, 32 or 64 (0: none has run)
};

template <class Upload>
inline void ilu_place(const IluHost& H, int nvar, int64_t n, int64_t blocks, MgArena& idx, MgArena& val, IluDev& g, Upload&& upload,
                      int64_t n_nodes = -1) {
  auto list = [&](const auto& v) {
    const size_t bytes = v.size() * sizeof(v[0]);
    void* at = idx.take(bytes);
    if (at && bytes) upload(at, (const void*)v.data(), bytes);
    return (decltype(v.data()))at;
  };
  auto vec = [&](int64_t doubles) { return (double*)val.take((size_t)doubles * sizeof(double)); };
  g = IluDev();
  g.n_colours = H.col.n_colours();
  g.pcol = list(H.pcol); g.nlow = list(H.nlow); g.colour = list(H.col.colour); g.nodes = list(H.col.nodes);
  if (!H.nown.empty()) g.nown = list(H.nown);
  g.cptr_host = H.col.cptr.data();
  g.val = vec(blocks * nvar * nvar); g.uinv = vec(n * nvar * nvar);
  const int64_t tail = std::max<int64_t>(std::max(n_nodes, n) * nvar, 1);
  g.ph = vec(tail); g.sh = vec(tail);
}

// foff of the fp32 copy (ilu_f32_node_floats per node, one behind the other): n + 1 entries
inline std::vector<int64_t> ilu_f32_offsets(int64_t n, const int64_t* bptr, const IluHost& H, int nvar) {
  std::vector<int64_t> foff((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = H.nown.empty() ? bptr[i + 1] - bptr[i] : (int64_t)H.nown[(size_t)i];
    foff[(size_t)i + 1] = foff[(size_t)i] + ilu_f32_node_floats(nvar, len, H.nlow[(size_t)i]);
  }
  return foff;
}

// The third allocation, measured and placed like the two of ilu_place: the offsets, then the floats (MgArena aligns both)
template <class Upload>
inline void ilu_place_f32(const std::vector<int64_t>& foff, MgArena& f32, IluDev& g, Upload&& upload) {
  const size_t bytes = foff.size() * sizeof(int64_t);
  void* at = f32.take(bytes);
  if (at) upload(at, (const void*)foff.data(), bytes);
  g.foff = (const int64_t*)at;
  g.val32 = (float*)f32.take((size_t)std::max<int64_t>(foff.back(), 1) * sizeof(float));
}

// ---- the iteration's scalars, its launch shapes and the layout of its work buffer: host code without HIP, so that a CPU build
// can test the layout (tests/host_solve_dist_shim.cpp) ----

// scalars of the iteration: they live in device memory and are consumed there; the host reads one copy per iteration
struct SolveScal {
  double rho, alpha, omega, beta;
  double rn2, rn2_plain, bn2, bn2_plain;   // ||r||^2 of the recurrence (or of the true residual after k_residual), plain form, rhs norms
  int32_t flag;                            // bit 0: alpha / omega / a norm is zero or not finite; bit 1: rho == 0
  int32_t bad_blocks;
  int32_t f32_overflow;                    // blocks of the fp32 copy that hold an entry which is not finite in fp32 (k_scale_f32)
  int32_t ilu_overflow;                    // entries of the ILU(0) factor that are finite in FP64 and not in fp32 (k_ilu_round_f32); this rank's own
};

constexpr int SPMV_NODES = 16;        // nodes per workgroup of k_spmv (256 threads)
constexpr int F32_LANES = 8;          // lanes per node of k_spmv_f32 and k_scale_f32
constexpr int F32_NODES = 32;         // nodes per workgroup of those two (256 threads)
constexpr int VEC_PER_BLOCK = 1024;   // vector entries per workgroup of the update kernels (256 threads x 4)
constexpr int DIST_RECORD = 8;        // doubles of the record a partitioned solve hands to allreduce_sum

enum Form { PLAIN, SCALED, F32 };   // what the fine operator applies: A, D^-1 A (both on the FP64 values), or the fp32 copy of D^-1 A

// Launch shapes: every grid size has its formula here and nowhere else
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t op_blocks(int64_t nodes, Form form) { return cdiv(nodes, form == F32 ? F32_NODES : SPMV_NODES); }   // k_spmv, k_spmv_f32, k_scale_f32
inline int64_t vec_blocks(int64_t entries) { return cdiv(entries, VEC_PER_BLOCK); }                                  // k_update_*

// What a partitioned solve (rdc_solve_dist) adds to the dimensions of a solve: ghost nodes behind the owned ones, the leading
// owned nodes whose rows have no ghost column (the operator runs over them while the exchange is in flight), the send list.
struct DistDims { int64_t n_nodes = 0, n_int = 0, n_send = 0; };

// workgroups, = pairs of dot-product partials, of one operator application: one range of rows, or the interior range and the
// rest one behind the other (n_int is no multiple of the nodes per workgroup)
inline int64_t op_parts(int64_t n_owned, int64_t n_int, Form form) { return op_blocks(n_int, form) + op_blocks(n_owned - n_int, form); }

// The work buffer of a solve: the one statement of its layout.  Without a base nothing is placed and `bytes` is what to allocate.
// dist: p and s get a ghost tail to receive into (n_nodes * nvar), partials cover the two row ranges, and the send buffer
// (n_send * nvar) and the record of the all-reduce follow; without it the layout is that of rdc_solve, byte for byte.
struct Work {
  double *r, *rh, *p, *v, *s, *t, *dinv, *partials, *send, *rec;
  SolveScal* scal;
  int64_t n, vec_blocks, node_blocks;
  size_t bytes;
};

inline Work carve(int nvar, int64_t n_owned, double* base, const DistDims* dist = nullptr) {
  Work w;
  w.n = n_owned * nvar;
  w.vec_blocks = vec_blocks(w.n);
  w.node_blocks = cdiv(n_owned, 256);
  const int64_t n = std::max<int64_t>(w.n, 1);
  const int64_t ng = dist ? std::max<int64_t>(dist->n_nodes * nvar, 1) : n;   // p and s: the operator reads their ghost entries
  // the largest set of partials a kernel leaves: (k_spmv, EPI 1), k_residual, k_update_xr
  const int64_t partials = std::max(std::max(2 * op_parts(n_owned, dist ? dist->n_int : 0, SCALED), 4 * w.node_blocks), 3 * w.vec_blocks) + 8;
  int64_t used = 0;
  auto take = [&](int64_t doubles) { double* at = base ? base + used : nullptr; used += doubles; return at; };
  w.r = take(n); w.rh = take(n); w.p = take(ng); w.v = take(n); w.s = take(ng); w.t = take(n);
  w.dinv = take(n * nvar);
  w.partials = take(partials);
  w.send = dist ? take(std::max<int64_t>(dist->n_send * nvar, 1)) : nullptr;
  w.rec = dist ? take(DIST_RECORD) : nullptr;
  w.scal = (SolveScal*)take(0);
  w.bytes = (size_t)used * sizeof(double) + sizeof(SolveScal);
  return w;
}

// The plan of a partitioned solve, checked on the host: every send id is an owned node, n_int lies in [0, n_owned], and no
// block of a node below n_int has a ghost column (bptr / bcol: the host copy of the pattern).  0 = fine; 1 = send id
// *where is not owned; 2 = n_int out of range; 3 = node *where below n_int has a ghost column.
inline int dist_plan_check(int64_t n_owned, const int64_t* bptr, const int32_t* bcol, int64_t n_int, int64_t n_send,
                           const int32_t* send_nodes, int64_t* where) {
  for (int64_t i = 0; i < n_send; i++)
    if (send_nodes[i] < 0 || send_nodes[i] >= n_owned) { *where = i; return 1; }
  if (n_int < 0 || n_int > n_owned) { *where = n_int; return 2; }
  for (int64_t node = 0; node < n_int; node++)
    for (int64_t k = bptr[node]; k < bptr[node + 1]; k++)
      if (bcol[k] >= n_owned) { *where = node; return 3; }
  return 0;
}

// ---- restarted GMRES(m) (option "solve_method" = 1): the small dense part of a cycle and the layout of its state,
// host+device and free of HIP, so that a CPU build can test exactly this code (tests/host_solve_gmres_shim.cpp) ----
constexpr int GMRES_MAX_RESTART = 128;      // largest "gmres_restart"
constexpr int GMRES_DEFAULT_RESTART = 30;   // PETSc's default

// flags of a step (GmresRec::flag)
enum {
  GMRES_NOT_FINITE = 1,     // an inner product, a norm or a rotation is not finite: the column was not taken
  GMRES_HAPPY = 2,          // h_{j+1,j} = 0: the Krylov space is exhausted, the column was taken and the cycle ends
  GMRES_SINGULAR = 4,       // the whole rotated column is zero (the operator is singular on the space): the column was not taken
  GMRES_Y_NOT_FINITE = 8    // the back substitution left an entry of y that is not finite: x was not updated
};

// what the host reads once per Arnoldi step (and once more behind the update of x)
struct GmresRec {
  double est;         // |g_{j+1}|: the residual norm the rotations claim
  double hnext;       // h_{j+1,j}
  double wn2;         // (w, w) before the orthogonalisation
  int32_t flag;
  int32_t overflow;   // entries of x whose update would not have been finite and that kept their value
};

// The Givens step of column j.  hcol: the raw column, entries 0 .. j + 1.  rcol: receives the column with the rotations 0 .. j - 1
// applied and the new rotation j formed on it (rcol[j] = the diagonal entry of R, rcol[j + 1] = 0).  cs, sn: the rotations;
// g: the rotated right-hand side, g[j + 1] is written and |g[j + 1]| is the residual estimate.  Returns 0, GMRES_NOT_FINITE (an
// entry of hcol, or the new diagonal entry, is not finite) or GMRES_SINGULAR (the rotated column is zero in rows j and j + 1); in
// the two latter cases cs, sn and g stay what they were, so that nothing non-finite is propagated.
RDC_SOLVE_HD int gmres_givens_step(int j, const double* hcol, double* rcol, double* cs, double* sn, double* g) {
  for (int i = 0; i <= j + 1; i++)
    if (!solve_finite(hcol[i])) return GMRES_NOT_FINITE;
  for (int i = 0; i <= j + 1; i++) rcol[i] = hcol[i];
  for (int i = 0; i < j; i++) {
    const double a = rcol[i], b = rcol[i + 1];
    rcol[i] = cs[i] * a + sn[i] * b;
    rcol[i + 1] = cs[i] * b - sn[i] * a;
  }
  const double a = rcol[j], b = rcol[j + 1];
  const double d = hypot(a, b);
  if (!solve_finite(d)) return GMRES_NOT_FINITE;
  if (d == 0.0) return GMRES_SINGULAR;
  const double c = a / d, s = b / d;
  cs[j] = c; sn[j] = s;
  rcol[j] = d; rcol[j + 1] = 0.0;
  g[j + 1] = -s * g[j];
  g[j] = c * g[j];
  return 0;
}

// y = R^-1 g for the leading k columns (R: column-major with leading dimension ld, upper triangular after the rotations).
// false: an entry of y is not finite (y is then unspecified and must not be used).
RDC_SOLVE_HD bool gmres_back_substitute(int ld, int k, const double* R, const double* g, double* y) {
  bool ok = true;
  for (int i = k - 1; i >= 0; i--) {
    double s = g[i];
    for (int l = i + 1; l < k; l++) s -= R[(int64_t)l * ld + i] * y[l];
    y[i] = s / R[(int64_t)i * ld + i];
    if (!solve_finite(y[i])) ok = false;
  }
  return ok;
}

// The state of GMRES on the device, an allocation of its own: the one statement of its layout.  Without a base nothing is placed
// and `bytes` is what to allocate.  m = restart.  V: the basis, m + 1 vectors of `stride` doubles (slot j + 1 also holds the raw
// w of step j); H: the raw Hessenberg matrix, R: its rotated form, both column-major (m + 1) x m; cs, sn [m]; g [m + 1]; y [m];
// hpass [m + 1]: the coefficients of the orthogonalisation pass at hand; scal: [0] = beta^2 of the start, [1] = 1 / h_{j+1,j},
// [2] = 1.0; partials: (m + 1) x vec_blocks, component-major (component c of workgroup b at c * vec_blocks + b); rec: the record.
// Across ranks (rdc_solve_dist_gmres; n_nodes >= n_owned given): a slot has the stride of a ghosted vector, n_nodes * nvar, so that
// the exchange of an operator application receives straight into the tail of v_j; every sum, scaling and combination still runs
// over the n owned entries of a slot and never touches its tail.  red [m + 2]: this rank's sums of a step, which the wide
// all-reduce turns into the global ones in place (j + 2 values of a Gram-Schmidt pass, or 1).  Without n_nodes there is no red and
// the layout is that of the single-partition solve, byte for byte.
struct GmresState {
  double *V, *H, *R, *cs, *sn, *g, *y, *hpass, *scal, *red, *partials;
  GmresRec* rec;
  int restart;
  int64_t n, stride, vec_blocks, partial_count;
  size_t basis_bytes, bytes;
  int cycles;   // out: the cycles of the last solve
};

constexpr int GMRES_SCALARS = 8;
constexpr int GMRES_WIDE_MAX = GMRES_MAX_RESTART + 2;   // what allreduce_sum_wide may be asked for at most (a step sums j + 2 <= restart + 1)

inline GmresState gmres_carve(int nvar, int64_t n_owned, int restart, double* base, int64_t n_nodes = -1) {
  GmresState g = GmresState();
  const int m = restart;
  g.restart = m;
  g.n = n_owned * nvar;
  g.stride = std::max<int64_t>(std::max(n_nodes, n_owned) * nvar, 1);
  g.vec_blocks = vec_blocks(g.n);
  g.partial_count = (int64_t)(m + 1) * std::max<int64_t>(g.vec_blocks, 1);
  int64_t used = 0;
  auto take = [&](int64_t doubles) { double* at = base ? base + used : nullptr; used += doubles; return at; };
  g.V = take((int64_t)(m + 1) * g.stride);
  g.basis_bytes = (size_t)used * sizeof(double);
  g.H = take((int64_t)(m + 1) * m); g.R = take((int64_t)(m + 1) * m);
  g.cs = take(m); g.sn = take(m); g.g = take(m + 1); g.y = take(m); g.hpass = take(m + 1);
  g.scal = take(GMRES_SCALARS);
  g.red = n_nodes >= 0 ? take(m + 2) : nullptr;
  g.partials = take(g.partial_count);
  g.rec = (GmresRec*)take((int64_t)(sizeof(GmresRec) / sizeof(double)));
  g.bytes = (size_t)used * sizeof(double);
  return g;
}
static_assert(sizeof(GmresRec) % sizeof(double) == 0, "the record is carved in doubles");

}  // namespace rdc

#if defined(__HIPCC__)
#include "../../include/rdc_assembly.h"
namespace rdc {

// what rdc_csr_matvec / rdc_solve need of a context (rdc_capi.hip fills it)
struct SolveDev {
  int nvar = 0;
  int64_t n_owned = 0, n_nodes = 0;
  const int64_t* bptr = nullptr;
  const int32_t* bcol = nullptr;
  const double* val = nullptr;
  const double* rhs = nullptr;
  double* work = nullptr;          // solve_work_bytes() bytes
  const int64_t* voff = nullptr;   // fp32 copy of D^-1 A: float offset of every owned node's values (n_owned + 1 entries) ...
  float* val32 = nullptr;          // ... and the values, voff[n_owned] floats (layout: f32_row_stride)
  SolveScal* host_rec = nullptr;   // pinned
  hipStream_t stream = nullptr;
  MgDev* mg = nullptr;             // the hierarchy (RDC_PRECOND_MULTIGRID only)
  const MgGsDev* gs = nullptr;     // its colour lists: the smoother is Gauss-Seidel (option "mg_smoother" = 1); null: damped Jacobi
  IluDev* ilu = nullptr;           // the factor (RDC_PRECOND_ILU0 and RDC_PRECOND_ILU0_LOCAL only)
  // partitioned solve (rdc_solve_dist) only.  comm == nullptr is the single-partition path.
  const rdc_solve_comm* comm = nullptr;
  int peers = 0;                                 // rdc_solve_dist_plan_peers
  const rdc_solve_comm_sized* sized = nullptr;   // rdc_solve_dist_mg: comm = &sized->base, and the exchange of the levels below the matrix
  DistDims dist;                       // n_nodes, interior nodes, length of the send list
  const int32_t* send_nodes = nullptr; // device copy of the send list (owned local node ids, send order)
  int* comm_rc = nullptr;              // out: the first non-zero return of a callback; nothing is called after it
  // restarted GMRES (option "solve_method" = 1, and rdc_solve_dist_gmres).  gmres == nullptr is BiCGStab, and nothing below is read.
  GmresState* gmres = nullptr;         // the state (gmres_carve), placed
  GmresRec* gmres_rec = nullptr;       // pinned: the record the host reads per Arnoldi step
  bool gmres_refine = false;           // option "gmres_refine": always a second Gram-Schmidt pass
  const rdc_solve_comm_wide* wide = nullptr;   // rdc_solve_dist_gmres: comm = &wide->sized.base, and the all-reduce of a step's sums
};

// what solve_run returns after a callback has failed (*SolveDev::comm_rc tells its value)
constexpr hipError_t SOLVE_COMM_FAILED = hipErrorOperatingSystem;

size_t solve_work_bytes(int nvar, int64_t n_owned, const DistDims* dist = nullptr);
hipError_t solve_matvec(const SolveDev& d, const double* x, double* y);
// mixed: iterate on the fp32 copy (built here from the current values); info->matrix_bits tells what the iteration streamed
hipError_t solve_run(const SolveDev& d, const rdc_solve_params& p, double* x, rdc_solve_info* info, bool mixed);
// D^-1 and the fp32 copy from the current values; synchronises to return the two counters
hipError_t solve_scale_f32(const SolveDev& d, int precond, int* bad_blocks, int* overflow);
hipError_t solve_matvec_f32(const SolveDev& d, const double* x, double* y);
// Test hook (rdc_solve_mg_apply): out = M in, one multigrid cycle behind the prologue of a multigrid solve (the same host function),
// in the form that solve would iterate in; in and out hold n_owned * nvar doubles and do not overlap; d.mg is set, d.comm is not.
// *bad_blocks > 0: a diagonal block of some level is not invertible, nothing was applied.  Synchronises.
hipError_t solve_mg_apply(const SolveDev& d, bool mixed, const double* in, double* out, int* bad_blocks, int* matrix_bits);
// Test hook (rdc_solve_ilu_apply, rdc_solve_ilu_local_apply): out = (LU)^-1 in behind the prologue of a solve with RDC_PRECOND_ILU0
// or, on lists with ghost columns, RDC_PRECOND_ILU0_LOCAL (the same host function);
// in and out hold n_owned * nvar doubles and do not overlap; d.ilu is set, d.comm is not.  *bad_blocks > 0: a diagonal block or a
// pivot U_ii is not invertible, nothing was applied.  Synchronises.
hipError_t solve_ilu_apply(const SolveDev& d, const double* in, double* out, int* bad_blocks);
// Test hook (rdc_solve_gmres_arnoldi): behind the prologue of a solve with `precond` (the same host function), v_0 = v0 / ||v0|| and
// `steps` Arnoldi steps with the kernels and the host loop of a cycle; d.gmres is set, d.mg / d.ilu as that solve needs them.  Copies
// the *steps_done + 1 basis vectors into V (device) and the raw Hessenberg matrix into H (host, (restart + 1) x restart, column-major).
// *bad_blocks > 0: nothing was run.  Synchronises.  With d.comm and d.wide (rdc_solve_dist_gmres_arnoldi): collective, v0 and V hold
// this rank's owned rows, the norm of v0 and every sum are global, H is the same on every rank.
hipError_t solve_gmres_arnoldi(const SolveDev& d, int precond, bool mixed, const double* v0, int steps, double* V, double* H,
                               int* steps_done, int* bad_blocks, int* matrix_bits);
// The pack kernel of the partitioned solves for a caller outside them (rdc_solid_newton_dist): send[i * nvar + a] =
// x[send_nodes[i] * nvar + a] for the n_send entries of the plan's device send list.  nvar 3 or 5; enqueues, does not synchronise.
hipError_t solve_halo_pack(int nvar, const int32_t* send_nodes, int64_t n_send, const double* x, double* send, hipStream_t stream);
// where the D^-1 of the last single-partition set-up lies in d.work (n_owned * nvar * nvar doubles)
const double* solve_dinv(const SolveDev& d);

}  // namespace rdc
#endif
#endif
