// rdc_solve.hip — device-resident linear solve on the context's own CSR values:
// block-pattern SpMV, node-block Jacobi, left-preconditioned BiCGStab.  FP64, gfx950, plain HIP C++.
//
// SpMV mapping: 16 lanes per node, 4 nodes per wave, 16 per workgroup.  The nvar rows of a node share one list of
// column nodes, so a lane computes its (block, unknown) position and gathers its x entry ONCE per 16-entry step and
// uses it for all nvar rows; per row the 16 lanes read 16 consecutive doubles (128 B) of the value stream, every value
// exactly once, non-temporal.  Tuned for the 15-block rows of the Kuhn meshes (75 entries = 5 steps, 94 % of the lanes
// busy); a row of any length just takes more steps.  A row sum is the lane's own entries in ascending order followed
// by a fixed xor butterfly over the 16 lanes: no atomics, no dependence on the launch shape, bitwise repeatable.
//
// Mixed precision (rdc_solve_mixed): k_scale_f32 stores fl32(D^-1 A) once per solve in a layout of its own (rdc_solve.h,
// f32_row_stride: rows padded to 16 bytes), and the two operator applications of an iteration stream that copy with
// k_spmv_f32: 8 lanes per node, 8 nodes per wave, 32 per workgroup; a lane reads 16 bytes (4 floats) per row and step, so
// the 8 lanes read 128 contiguous bytes per row like the 16 lanes of k_spmv do, and it gathers its 4 x entries once for
// all nvar rows.  x, y and every sum are FP64; the sum order is the lane's own entries ascending, then a fixed xor
// butterfly over the 8 lanes.  No D^-1 epilogue: the copy is already scaled.  Everything that decides or reports (first
// residual, every confirmation / restart, closing residual, norms) stays on k_spmv + k_residual over the FP64 values.
//
// Multigrid (precond 3): a V(1,1) cycle over aggregation levels, applied from the RIGHT (v = A^ M p, t = A^ M s,
// x += alpha M p + omega M s), so the recurrence residual and everything that decides stay what they are above.  Coarse
// matrices live in the same node-block layout and go through k_spmv and k_precond_setup as they are; k_galerkin rebuilds
// their values per solve (a gather in a fixed order: no atomics), k_restrict / k_prolong / k_smooth are the rest of the cycle.
// The cycle has no inner product and no host round trip.  Its smoother is an argument (SolveDev::gs): damped block Jacobi, or,
// opt-in, forward Gauss-Seidel in a multicolour order (k_gs and its kin, further down) for every sweep but the first of a level.
//
// Block ILU(0) (precond 4): the other right preconditioner of `iteration`, M = (LU)^-1 with LU the block ILU(0) of
// D^-1 A in the multicolour order of the Gauss-Seidel smoother; factorisation, forward and backward sweep are one launch per colour
// each (k_ilu_copy, k_ilu_factor, k_ilu_fwd, k_ilu_bwd, further down), on a copy of D^-1 A in a layout of its own (rdc_solve.h).
// Rank-local (precond 5, rdc_solve_dist): the same of the owned square of D^-1 A, rows and columns below n_owned, through the _owned
// forms of those kernels, which end every row at its owned positions; the apply exchanges nothing, M p and M s travel in the two
// exchanges of the iteration.
//
// Dot products: per-workgroup partials (wave butterfly, then the four waves in order) into a scratch array, then one
// small kernel that adds the partials in a fixed order AND turns them into the next scalar (alpha, omega, beta) in
// device memory.  No floating-point atomics anywhere.
//
// Across partitions (rdc_solve_dist): the same driver with a communicator.  apply_halo wraps an operator application
// into pack / exchange_begin / rows without ghost columns / exchange_end / the other rows, and k_finalize becomes k_reduce, the
// all-reduce callback and k_advance, so that every scalar the host reads and every branch it takes is global.  Without a
// communicator the launches are those of the single-partition path, in the same order.  Multigrid across ranks (rdc_solve_dist_mg):
// aggregates stay inside a partition, every level has a ghost layer (rdc_solve.h, MgHalo), mg_apply exchanges the argument of every
// operator application inside the cycle, and on the levels below the matrix the kernel that last writes a vector also fills the
// level's send buffer (k_restrict_pack, k_prolong_pack, k_smooth_pack), so that a coarse exchange costs no launch.
//
// Restarted GMRES(m) (option "solve_method" = 1): the second Krylov method of rdc_solve and rdc_solve_mixed, on the same
// system with the same right preconditioners.  Its orthogonalisation is two launches per step, k_gmres_dots (all inner products
// of a step, every basis vector read once) and k_gmres_orth (the update, every basis vector read once); k_gmres_finalize sums
// their partials in a fixed order and runs the Givens step in device memory, and the host reads one record per step.  Its state
// is an allocation of its own (rdc_solve.h, gmres_carve).  Across ranks (rdc_solve_dist_gmres): the same driver with a communicator,
// as for BiCGStab.  The basis slots get the stride of a ghosted vector, so that apply_halo receives straight into the tail of v_j
// (one k_halo_pack per step fills the send buffer; the pack is not folded into k_gmres_scale, which would need the node-to-slot
// lists of the plan on the device); k_gmres_finalize becomes k_gmres_reduce, the wide all-reduce callback and k_gmres_advance, two
// per step (three with "gmres_refine"); the overflow counter of the update of x rides in the record of the true residual behind it.
//
// Host side (below the kernels): `iteration` is the one BiCGStab iteration (fp32 copy, multigrid cycle and communicator are
// arguments), `apply` the one entry to y = A_l x on any level in any form; `carve` (rdc_solve.h) is the one statement of the work
// buffer's layout.  `open_solve` is what every solve does before its first iteration, `run` the BiCGStab driver, `run_gmres` the
// GMRES driver with `gmres_step` as its one Arnoldi step.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "rdc_solve.h"

namespace rdc {
namespace {

// (workgroup shapes of the kernels: SPMV_NODES, F32_LANES, F32_NODES, VEC_PER_BLOCK in rdc_solve.h, beside the launch formulas)
constexpr int MAX_BREAKDOWNS = 10;    // restarts after a break-down before RDC_SOLVE_BREAKDOWN

enum { STAGE_INIT = 0, STAGE_ALPHA = 1, STAGE_OMEGA = 2, STAGE_RHO = 3 };

__device__ __forceinline__ bool finite_d(double x) { return solve_finite(x); }

// sums `NC` values over the workgroup in a fixed order and lets thread 0 store them to out[blockIdx.x * NC + c]
template <int NC>
__device__ __forceinline__ void block_partials(double (&c)[NC], double* __restrict__ out) {
  __shared__ double sh[NC][4];
#pragma unroll
  for (int i = 0; i < NC; i++)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c[i] += __shfl_xor(c[i], off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int i = 0; i < NC; i++) sh[i][wave] = c[i];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < NC; i++) out[(size_t)blockIdx.x * NC + i] = ((sh[i][0] + sh[i][1]) + sh[i][2]) + sh[i][3];
}

// y = A x (EPI 0), y = D^-1 (A x) with the partials of (y, w) and (y, y) (EPI 1), or y = D^-1 (A x) alone (EPI 2)
template <int NV, int EPI>
__global__ __launch_bounds__(256) void k_spmv(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                              const double* __restrict__ val, const double* __restrict__ x,
                                              double* __restrict__ y, int64_t n_owned, const double* __restrict__ dinv,
                                              const double* __restrict__ w, double* __restrict__ partials) {
  const int lane = threadIdx.x & 15;
  const int64_t node = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  const bool live = node < n_owned;
  double acc[NV];
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  if (live) {
    const int64_t b0 = bptr[node];
    const int L = (int)(bptr[node + 1] - b0) * NV;      // entries of one row of the node
    const double* __restrict__ vrow = val + (int64_t)NV * NV * b0;
    for (int j = lane; j < L; j += 16) {
      const int k = j / NV, b = j - k * NV;
      const double xv = x[(int64_t)bcol[b0 + k] * NV + b];
#pragma unroll
      for (int a = 0; a < NV; a++) acc[a] = fma(__builtin_nontemporal_load(vrow + (int64_t)a * L + j), xv, acc[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) acc[a] += __shfl_xor(acc[a], off, 16);
  if (EPI == 0) {
    double out = acc[0];
#pragma unroll
    for (int a = 1; a < NV; a++) out = lane == a ? acc[a] : out;
    if (live && lane < NV) y[node * NV + lane] = out;
  } else {
    double c[2] = {0.0, 0.0};
    if (live && lane < NV) {
      const double* __restrict__ drow = dinv + (node * NV + lane) * NV;
      double z = 0.0;
#pragma unroll
      for (int a = 0; a < NV; a++) z = fma(drow[a], acc[a], z);
      y[node * NV + lane] = z;
      if (EPI == 1) {
        c[0] = z * w[node * NV + lane];
        c[1] = z * z;
      }
    }
    if (EPI == 1) block_partials<2>(c, partials);
  }
}

// D^-1 of every owned node from the CSR values (one thread per node); counts the blocks it could not invert
template <int NV>
__global__ __launch_bounds__(256) void k_precond_setup(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                       const double* __restrict__ val, int64_t n_owned, int precond,
                                                       double* __restrict__ dinv, SolveScal* __restrict__ scal) {
  const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= n_owned) return;
  const int64_t kd = csr_diag_block(bptr, bcol, node);
  double d[NV][NV];
  bool ok = kd >= 0;
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int b = 0; b < NV; b++) d[a][b] = ok ? val[csr_value_offset(bptr, NV, node, a, kd, b)] : 0.0;
  ok = precond_block<NV>(d, ok ? precond : 2) && ok;
  if (!ok) atomicAdd(&scal->bad_blocks, 1);
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int b = 0; b < NV; b++) dinv[(node * NV + a) * NV + b] = d[a][b];
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// fp32 copy of D^-1 A (layout: rdc_solve.h, f32_row_stride): 8 lanes per node, a lane takes the blocks k = lane, lane + 8, ...
// Reads every FP64 value once (non-temporal), multiplies the block by D^-1 of the node from the left, stores the floats
// and the zero padding of every row; counts the blocks with an entry that is not finite in fp32.  Runs after k_precond_setup.
template <int NV>
__global__ __launch_bounds__(256) void k_scale_f32(const int64_t* __restrict__ bptr, const int64_t* __restrict__ voff,
                                                   const double* __restrict__ val, const double* __restrict__ dinv,
                                                   int64_t n_owned, float* __restrict__ val32, SolveScal* __restrict__ scal) {
  const int lane = threadIdx.x & (F32_LANES - 1);
  const int64_t node = (int64_t)blockIdx.x * F32_NODES + (threadIdx.x / F32_LANES);
  if (node >= n_owned) return;
  const int64_t b0 = bptr[node];
  const int len = (int)(bptr[node + 1] - b0);
  const int L = len * NV, Lp = (int)f32_row_stride(NV, len);
  const double* __restrict__ vrow = val + (int64_t)NV * NV * b0;
  float* __restrict__ orow = val32 + voff[node];
  double di[NV][NV];
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int b = 0; b < NV; b++) di[a][b] = dinv[(node * NV + a) * NV + b];
  int bad = 0;
  for (int k = lane; k < len; k += F32_LANES) {
    double blk[NV][NV];
    float out[NV][NV];
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) blk[a][b] = __builtin_nontemporal_load(vrow + ((int64_t)a * len + k) * NV + b);
    if (!scaled_block_f32<NV>(di, blk, out)) bad++;
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) orow[(int64_t)a * Lp + k * NV + b] = out[a][b];
  }
  if (lane < Lp - L)   // at most 3 padding floats per row
#pragma unroll
    for (int a = 0; a < NV; a++) orow[(int64_t)a * Lp + L + lane] = 0.0f;
  if (bad) atomicAdd(&scal->f32_overflow, bad);
}

// y = A32 x on the fp32 copy (EPI 0), with the partials of (y, w) and (y, y) (EPI 1); x, y and the sums are FP64
template <int NV, int EPI>
__global__ __launch_bounds__(256) void k_spmv_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                  const int64_t* __restrict__ voff, const float* __restrict__ val32,
                                                  const double* __restrict__ x, double* __restrict__ y, int64_t n_owned,
                                                  const double* __restrict__ w, double* __restrict__ partials) {
  const int lane = threadIdx.x & (F32_LANES - 1);
  const int64_t node = (int64_t)blockIdx.x * F32_NODES + (threadIdx.x / F32_LANES);
  const bool live = node < n_owned;
  double acc[NV];
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  const int64_t b0 = live ? bptr[node] : 0;
  const int len = live ? (int)(bptr[node + 1] - b0) : 0;
  if (len > 0) {
    const int L = len * NV, Lp = (int)f32_row_stride(NV, len);   // entries of one row of the node, and its padded stride
    const float* __restrict__ vrow = val32 + voff[node];
    // x indices of the 4 entries at j .. j + 3.  Every load of the loop is unconditional -- a position past the row's end
    // (padding, or the look-ahead behind the last step) re-reads the row's last entry and is zeroed or dropped afterwards:
    // a load behind a per-element condition would be branched around and waited for one by one.
    auto columns = [&](int j, int32_t (&cn)[4], int (&cb)[4]) {   // column node and unknown of the entries j .. j + 3
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int jj = min(j + e, L - 1), k = jj / NV;
        cb[e] = jj - k * NV;
        cn[e] = bcol[b0 + k];
      }
    };
    int32_t cn[4], nn[4];
    int cb[4], nb[4];
    columns(4 * lane, cn, cb);
    for (int j = 4 * lane; j < Lp; j += 4 * F32_LANES) {
      // the next step's column nodes are requested together with this step's values and x entries and used a step later:
      // the bcol -> x chain then costs one memory latency per step, not two
      columns(j + 4 * F32_LANES, nn, nb);
      f32x4 v[NV];
#pragma unroll
      for (int a = 0; a < NV; a++) v[a] = __builtin_nontemporal_load((const f32x4*)(vrow + (int64_t)a * Lp + j));
      double xv[4];
#pragma unroll
      for (int e = 0; e < 4; e++) xv[e] = x[(int64_t)cn[e] * NV + cb[e]];
      __builtin_amdgcn_sched_barrier(0);   // keep the three groups of loads ahead of the arithmetic
#pragma unroll
      for (int e = 0; e < 4; e++) {
        xv[e] = j + e < L ? xv[e] : 0.0;
        cn[e] = nn[e];
        cb[e] = nb[e];
      }
#pragma unroll
      for (int a = 0; a < NV; a++) {
        acc[a] = fma((double)v[a].x, xv[0], acc[a]);
        acc[a] = fma((double)v[a].y, xv[1], acc[a]);
        acc[a] = fma((double)v[a].z, xv[2], acc[a]);
        acc[a] = fma((double)v[a].w, xv[3], acc[a]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int off = F32_LANES / 2; off >= 1; off >>= 1) acc[a] += __shfl_xor(acc[a], off, F32_LANES);
  double out = acc[0];
#pragma unroll
  for (int a = 1; a < NV; a++) out = lane == a ? acc[a] : out;
  if (live && lane < NV) y[node * NV + lane] = out;
  if (EPI == 1) {
    double c[2] = {0.0, 0.0};
    if (live && lane < NV) {
      c[0] = out * w[node * NV + lane];
      c[1] = out * out;
    }
    block_partials<2>(c, partials);
  }
}

// r = r_hat = D^-1 (scale * rhs - ax), p = v = 0; partials of ||r||^2, ||scale*rhs - ax||^2, ||D^-1 b||^2, ||b||^2
template <int NV>
__global__ __launch_bounds__(256) void k_residual(const double* __restrict__ rhs, double scale, const double* __restrict__ ax,
                                                  const double* __restrict__ dinv, double* __restrict__ r, double* __restrict__ rh,
                                                  double* __restrict__ p, double* __restrict__ v, int64_t n_owned,
                                                  double* __restrict__ partials) {
  const int64_t node = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double c[4] = {0.0, 0.0, 0.0, 0.0};
  if (node < n_owned) {
    double b[NV], res[NV];
#pragma unroll
    for (int a = 0; a < NV; a++) {
      b[a] = scale * rhs[node * NV + a];
      res[a] = b[a] - ax[node * NV + a];
      c[1] = fma(res[a], res[a], c[1]);
      c[3] = fma(b[a], b[a], c[3]);
    }
#pragma unroll
    for (int a = 0; a < NV; a++) {
      double zr = 0.0, zb = 0.0;
#pragma unroll
      for (int q = 0; q < NV; q++) {
        const double dq = dinv[(node * NV + a) * NV + q];
        zr = fma(dq, res[q], zr);
        zb = fma(dq, b[q], zb);
      }
      r[node * NV + a] = zr;
      rh[node * NV + a] = zr;
      p[node * NV + a] = 0.0;
      v[node * NV + a] = 0.0;
      c[0] = fma(zr, zr, c[0]);
      c[2] = fma(zb, zb, c[2]);
    }
  }
  block_partials<4>(c, partials);
}

// the `ncomp` sums of the partials of the previous kernel, in a fixed order (one workgroup of 1024): thread 0 finds them in
// sh[c][0] behind the call, 0.0 in the components from ncomp on.  skip: a flagged iteration wrote no partials, nothing is read.
__device__ __forceinline__ void sum_partials(const double* __restrict__ partials, int64_t nparts, int ncomp, bool skip,
                                             double (&sh)[4][1024]) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (!skip)
    for (int64_t i = threadIdx.x; i < nparts; i += 1024)
      for (int c = 0; c < ncomp; c++) s[c] += partials[i * ncomp + c];
  for (int c = 0; c < 4; c++) sh[c][threadIdx.x] = s[c];
  __syncthreads();
  for (int off = 512; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int c = 0; c < ncomp; c++) sh[c][threadIdx.x] += sh[c][threadIdx.x + off];
    __syncthreads();
  }
}

// The scalars of the iteration from the sums of a stage: the one statement of rho, alpha, omega, beta and the flags.  The sums
// are those of the whole system: of this partition's partials (k_finalize), or of all partitions (k_advance).
__device__ __forceinline__ void advance_scalars(SolveScal* __restrict__ scal, int stage, double s0, double s1, double s2, double s3) {
  if (stage == STAGE_INIT) {
    scal->rn2 = s0; scal->rn2_plain = s1; scal->bn2 = s2; scal->bn2_plain = s3;
    scal->rho = s0; scal->alpha = 1.0; scal->omega = 1.0; scal->beta = 0.0;   // p = v = 0: the first update gives p = r
    scal->flag = (finite_d(s0) && finite_d(s2)) ? 0 : 1;
  } else if (stage == STAGE_ALPHA) {
    const double alpha = scal->rho / s0;
    scal->alpha = alpha;
    if (s0 == 0.0 || !finite_d(alpha)) scal->flag |= 1;
  } else if (stage == STAGE_OMEGA) {
    const double omega = s1 > 0.0 ? s0 / s1 : 0.0;
    scal->omega = omega;
    if (omega == 0.0 || !finite_d(omega)) scal->flag |= 1;
  } else {
    const double beta = (s0 / scal->rho) * (scal->alpha / scal->omega);
    scal->rn2 = s1; scal->beta = beta; scal->rho = s0;
    if (!finite_d(s1) || !finite_d(beta) || s2 != 0.0) scal->flag |= 1;
    else if (s0 == 0.0) scal->flag |= 2;
  }
}

// adds the partials of the previous kernel in a fixed order and advances the scalars (one workgroup)
__global__ __launch_bounds__(1024) void k_finalize(const double* __restrict__ partials, int64_t nparts, int ncomp, int stage,
                                                   SolveScal* __restrict__ scal) {
  __shared__ double sh[4][1024];
  const bool skip = stage != STAGE_INIT && scal->flag != 0;   // a flagged iteration wrote no partials
  sum_partials(partials, nparts, ncomp, skip, sh);
  if (threadIdx.x != 0 || skip) return;
  advance_scalars(scal, stage, sh[0][0], sh[1][0], sh[2][0], sh[3][0]);
}

// Partitioned solve: k_finalize in two halves with the all-reduce between them.  k_reduce: this partition's sums, in the same
// fixed order, into rec[0 .. 4); counters (the first residual of a solve): rec[4], rec[5] = this partition's bad_blocks and
// f32_overflow, counts as doubles (exact below 2^53).  A flagged iteration (the flag is the same on every partition) sends zeros.
// extra (GMRES across ranks, the true residual behind an update of x; never with counters): rec[4] = this partition's count of
// entries of x that kept their value (GmresRec::overflow), so that it becomes global in the same all-reduce.
__global__ __launch_bounds__(1024) void k_reduce(const double* __restrict__ partials, int64_t nparts, int ncomp, int stage,
                                                 const SolveScal* __restrict__ scal, double* __restrict__ rec, int counters,
                                                 const int32_t* __restrict__ extra) {
  __shared__ double sh[4][1024];
  const bool skip = stage != STAGE_INIT && scal->flag != 0;
  sum_partials(partials, nparts, ncomp, skip, sh);
  if (threadIdx.x != 0) return;
  for (int c = 0; c < 4; c++) rec[c] = sh[c][0];
  rec[4] = counters ? (double)scal->bad_blocks : extra ? (double)*extra : 0.0;
  rec[5] = counters ? (double)scal->f32_overflow : 0.0;
  rec[6] = 0.0; rec[7] = 0.0;
}

// k_advance: the scalars from the all-reduced record (one thread).  Every partition computes the same bits from the same bits.
__global__ void k_advance(const double* __restrict__ rec, int stage, SolveScal* __restrict__ scal, int counters, int32_t* __restrict__ extra) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (extra) *extra = rec[4] < 2147483647.0 ? (int32_t)rec[4] : 2147483647;   // the global count, saturated
  if (stage != STAGE_INIT && scal->flag != 0) return;
  if (counters) {
    scal->bad_blocks = (int32_t)rec[4];
    scal->f32_overflow = (int32_t)rec[5];
  }
  advance_scalars(scal, stage, rec[0], rec[1], rec[2], rec[3]);
}

// send[i * NV + a] = x[send_nodes[i] * NV + a]: the owned values the peers hold as ghosts, in plan order (one thread per double)
template <int NV>
__global__ __launch_bounds__(256) void k_halo_pack(const int32_t* __restrict__ send_nodes, int64_t n_send, const double* __restrict__ x,
                                                   double* __restrict__ send) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_send * NV) return;
  const int64_t e = i / NV;
  send[i] = x[(int64_t)send_nodes[e] * NV + (i - e * NV)];
}

// p = r + beta (p - omega v)
__global__ __launch_bounds__(256) void k_update_p(const double* __restrict__ r, double* __restrict__ p, const double* __restrict__ v,
                                                  const SolveScal* __restrict__ scal, int64_t n) {
  const double beta = scal->beta, omega = scal->omega;
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) p[i] = r[i] + beta * (p[i] - omega * v[i]);
  }
}

// s = r - alpha v
__global__ __launch_bounds__(256) void k_update_s(const double* __restrict__ r, const double* __restrict__ v, double* __restrict__ s,
                                                  const SolveScal* __restrict__ scal, int64_t n) {
  if (scal->flag) return;
  const double alpha = scal->alpha;
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) s[i] = r[i] - alpha * v[i];
  }
}

// x += alpha p + omega s, r = s - omega t, partials of (r_hat, r) and ||r||^2.  An entry of x whose update would not be
// finite (overflow: p, s, t themselves are finite when alpha and omega passed their checks) keeps its value and is counted;
// the count flags the iteration, so x never holds a NaN or inf that the solver wrote.
// RIGHT (multigrid): x advances along the preconditioned directions px = M p and sx = M s, r stays s - omega t.
template <bool RIGHT>
__global__ __launch_bounds__(256) void k_update_xr(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                   const double* __restrict__ s, const double* __restrict__ t,
                                                   const double* __restrict__ rh, const SolveScal* __restrict__ scal, int64_t n,
                                                   double* __restrict__ partials, const double* __restrict__ px,
                                                   const double* __restrict__ sx) {
  if (scal->flag) return;   // uniform: alpha or omega is unusable, x and r stay what they were
  const double alpha = scal->alpha, omega = scal->omega;
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
  double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) {
      const double si = s[i];
      const double xn = RIGHT ? x[i] + (alpha * px[i] + omega * sx[i]) : x[i] + (alpha * p[i] + omega * si);
      if (finite_d(xn)) x[i] = xn;
      else c[2] += 1.0;
      const double ri = si - omega * t[i];
      r[i] = ri;
      c[0] = fma(rh[i], ri, c[0]);
      c[1] = fma(ri, ri, c[1]);
    }
  }
  block_partials<3>(c, partials);
}

// ---- multigrid: Galerkin product, restriction, prolongation, smoother ----

// Values of a coarse level from those of the level above it: coarse block c is the sum of the fine blocks cidx[cptr[c] ..
// cptr[c + 1]) in list order (ascending fine node, then block).  One thread per (coarse block, entry): thread g of the grid
// owns entry (a, b) = ((g % NV^2) / NV, g % NV) of coarse block g / NV^2 whatever the launch shape, and adds its
// contributions from 0.0 in list order: no atomics, two runs bitwise equal.  SCALE (level 0 -> 1): the summand is
// D^-1_n A_nm (scaled_entry: FP64, ascending, no contraction); the NV lanes of a block column then read the same NV values
// in one instruction, so the FP64 stream still crosses the memory bus once (non-temporal, as k_scale_f32 reads it).
template <int NV, bool SCALE>
__global__ __launch_bounds__(256) void k_galerkin(const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
                                                  const int32_t* __restrict__ cnode, const int32_t* __restrict__ brow,
                                                  int64_t coarse_blocks, const int64_t* __restrict__ fbptr,
                                                  const double* __restrict__ fval, const double* __restrict__ fdinv,
                                                  const int64_t* __restrict__ cbptr, double* __restrict__ cval) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = g / (NV * NV);
  if (c >= coarse_blocks) return;
  const int e = (int)(g - c * (NV * NV)), a = e / NV, b = e - a * NV;
  double s = 0.0;
  const int64_t i1 = cptr[c + 1];
  for (int64_t i = cptr[c]; i < i1; i++) {
    const int64_t n = cnode[i], fb0 = fbptr[n], flen = fbptr[n + 1] - fb0;
    const double* __restrict__ base = fval + (int64_t)NV * NV * fb0 + ((int64_t)cidx[i] - fb0) * NV + b;   // entry (0, b) of the fine block
    if (SCALE) {
      double drow[NV], acol[NV];
#pragma unroll
      for (int q = 0; q < NV; q++) {
        drow[q] = fdinv[(n * NV + a) * NV + q];
        acol[q] = __builtin_nontemporal_load(base + (int64_t)q * flen * NV);
      }
      s = s + scaled_entry<NV>(drow, acol);
    } else {
      s = s + __builtin_nontemporal_load(base + (int64_t)a * flen * NV);
    }
  }
  const int64_t I = brow[c], cb0 = cbptr[I], clen = cbptr[I + 1] - cb0;
  cval[(int64_t)NV * NV * cb0 + ((int64_t)a * clen + (c - cb0)) * NV + b] = s;
}

// Across ranks (PACK, levels below the matrix): the kernel that last writes a vector which is exchanged next also writes that
// node's entries of the level's send buffer, so that a coarse exchange costs no launch of its own.  send_slot[send_ptr[n] ..
// send_ptr[n + 1]) are the slots of node n (one per peer that holds it as a ghost, usually none): entry (slot, a) gets the value
// the thread has just stored to x, from its register -- no thread reads what another wrote.
struct SendList {
  const int64_t* ptr;
  const int32_t* slot;
  double* buf;
};

template <int NV>
__device__ __forceinline__ void pack_entry(const SendList& s, int64_t node, int a, double value) {
  const int64_t s1 = s.ptr[node + 1];
  for (int64_t i = s.ptr[node]; i < s1; i++) s.buf[(int64_t)s.slot[i] * NV + a] = value;
}

// r_c = P^T (r - t) and the first smoothing sweep of the coarse level, x_c = w D_c^-1 r_c: one thread per aggregate, its
// members in ascending order
template <int NV, bool PACK>
__device__ __forceinline__ void restrict_body(const int64_t* __restrict__ mptr, const int32_t* __restrict__ member,
                                              const double* __restrict__ r, const double* __restrict__ t,
                                              const double* __restrict__ cdinv, double omega, int64_t n_coarse,
                                              double* __restrict__ rc, double* __restrict__ xc, const SendList& send) {
  const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (I >= n_coarse) return;
  double acc[NV];
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  const int64_t m1 = mptr[I + 1];
  for (int64_t m = mptr[I]; m < m1; m++) {
    const int64_t n = member[m];
#pragma unroll
    for (int a = 0; a < NV; a++) acc[a] += r[n * NV + a] - t[n * NV + a];
  }
#pragma unroll
  for (int a = 0; a < NV; a++) {
    double z = 0.0;
#pragma unroll
    for (int q = 0; q < NV; q++) z = fma(cdinv[(I * NV + a) * NV + q], acc[q], z);
    rc[I * NV + a] = acc[a];
    xc[I * NV + a] = omega * z;
    if (PACK) pack_entry<NV>(send, I, a, omega * z);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void k_restrict(const int64_t* __restrict__ mptr, const int32_t* __restrict__ member,
                                                  const double* __restrict__ r, const double* __restrict__ t,
                                                  const double* __restrict__ cdinv, double omega, int64_t n_coarse,
                                                  double* __restrict__ rc, double* __restrict__ xc) {
  restrict_body<NV, false>(mptr, member, r, t, cdinv, omega, n_coarse, rc, xc, SendList{});
}

template <int NV>
__global__ __launch_bounds__(256) void k_restrict_pack(const int64_t* __restrict__ mptr, const int32_t* __restrict__ member,
                                                       const double* __restrict__ r, const double* __restrict__ t,
                                                       const double* __restrict__ cdinv, double omega, int64_t n_coarse,
                                                       double* __restrict__ rc, double* __restrict__ xc, SendList send) {
  restrict_body<NV, true>(mptr, member, r, t, cdinv, omega, n_coarse, rc, xc, send);
}

// x += P x_c: one thread per fine unknown, one read of agg[n]
template <int NV, bool PACK>
__device__ __forceinline__ void prolong_body(const int32_t* __restrict__ agg, const double* __restrict__ xc, double* __restrict__ x,
                                             int64_t n_fine, const SendList& send) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_fine * NV) return;
  const int64_t n = i / NV;
  const double xn = x[i] + xc[(int64_t)agg[n] * NV + (i - n * NV)];
  x[i] = xn;
  if (PACK) pack_entry<NV>(send, n, (int)(i - n * NV), xn);
}

template <int NV>
__global__ __launch_bounds__(256) void k_prolong(const int32_t* __restrict__ agg, const double* __restrict__ xc, double* __restrict__ x,
                                                 int64_t n_fine) {
  prolong_body<NV, false>(agg, xc, x, n_fine, SendList{});
}

template <int NV>
__global__ __launch_bounds__(256) void k_prolong_pack(const int32_t* __restrict__ agg, const double* __restrict__ xc,
                                                      double* __restrict__ x, int64_t n_fine, SendList send) {
  prolong_body<NV, true>(agg, xc, x, n_fine, send);
}

// damped block Jacobi, one thread per unknown: x = w D^-1 r (FIRST) or x += w D^-1 (r - t); IDENT: D = I (level 0, whose
// operator D^-1 A has the identity on its block diagonal)
template <int NV, bool IDENT, bool FIRST, bool PACK>
__device__ __forceinline__ void smooth_body(const double* __restrict__ dinv, const double* __restrict__ r, const double* __restrict__ t,
                                            double omega, int64_t n, double* __restrict__ x, const SendList& send) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * NV) return;
  const int64_t node = i / NV;
  double z;
  if (IDENT) {
    z = FIRST ? r[i] : r[i] - t[i];
  } else {
    z = 0.0;
#pragma unroll
    for (int q = 0; q < NV; q++) {
      const double res = FIRST ? r[node * NV + q] : r[node * NV + q] - t[node * NV + q];
      z = fma(dinv[i * NV + q], res, z);
    }
  }
  const double xn = FIRST ? omega * z : x[i] + omega * z;
  x[i] = xn;
  if (PACK) pack_entry<NV>(send, node, (int)(i - node * NV), xn);
}

template <int NV, bool IDENT, bool FIRST>
__global__ __launch_bounds__(256) void k_smooth(const double* __restrict__ dinv, const double* __restrict__ r, const double* __restrict__ t,
                                                double omega, int64_t n, double* __restrict__ x) {
  smooth_body<NV, IDENT, FIRST, false>(dinv, r, t, omega, n, x, SendList{});
}

// the sweeps on a level below the matrix across ranks
template <int NV>
__global__ __launch_bounds__(256) void k_smooth_pack(const double* __restrict__ dinv, const double* __restrict__ r,
                                                     const double* __restrict__ t, double omega, int64_t n, double* __restrict__ x,
                                                     SendList send) {
  smooth_body<NV, false, false, true>(dinv, r, t, omega, n, x, send);
}

// ---- multicolour Gauss-Seidel smoother (option "mg_smoother" = 1): x_n += D_l^-1 (r_n - (A_l x)_n), colour after colour ----
//
// A sweep visits the colour lists of the level in order (rdc_solve.h, mg_colour).  No two nodes of a colour are coupled, so the
// nodes of a colour neither read nor write each other's entries of x and can run in any order: what orders the sweep is the
// boundary between two colours -- a launch boundary (k_gs, k_gs_f32: one launch per colour), or, on a level small enough for
// one workgroup, the barrier between two colours of one launch (k_gs_fused, k_gs_f32_fused).  x is read and written in place
// and therefore neither const nor __restrict__ here; a node reads its own entries (its diagonal block) before it writes them:
// the write of a lane depends on the sums of all lanes of the node through the butterfly.  The arithmetic of a node is
// row_product followed by that of k_smooth with a damping of 1, in both kinds of launch: their results are bitwise equal.

// The row product of k_spmv for one node: acc[a] = row a of `node` times x, a = 0 .. NV-1, in all 16 lanes of the node -- a lane's
// own entries in ascending order, then the xor butterfly over the 16 lanes.  Every lane of the node calls, live or not (the
// butterfly).  Stated a second time, for an x that is written in place: k_spmv keeps its own text, so that its device assembly
// stays what it was.
template <int NV>
__device__ __forceinline__ void row_product(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                            const double* __restrict__ val, const double* x, int64_t node, bool live, int lane,
                                            double (&acc)[NV]) {
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  if (live) {
    const int64_t b0 = bptr[node];
    const int L = (int)(bptr[node + 1] - b0) * NV;      // entries of one row of the node
    const double* __restrict__ vrow = val + (int64_t)NV * NV * b0;
    for (int j = lane; j < L; j += 16) {
      const int k = j / NV, b = j - k * NV;
      const double xv = x[(int64_t)bcol[b0 + k] * NV + b];
#pragma unroll
      for (int a = 0; a < NV; a++) acc[a] = fma(__builtin_nontemporal_load(vrow + (int64_t)a * L + j), xv, acc[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) acc[a] += __shfl_xor(acc[a], off, 16);
}

// ... and that of k_spmv_f32: 8 lanes per node, 16 bytes per lane, row and step; x and the sums are FP64
template <int NV>
__device__ __forceinline__ void row_product_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                const int64_t* __restrict__ voff, const float* __restrict__ val32, const double* x,
                                                int64_t node, bool live, int lane, double (&acc)[NV]) {
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  const int64_t b0 = live ? bptr[node] : 0;
  const int len = live ? (int)(bptr[node + 1] - b0) : 0;
  if (len > 0) {
    const int L = len * NV, Lp = (int)f32_row_stride(NV, len);   // entries of one row of the node, and its padded stride
    const float* __restrict__ vrow = val32 + voff[node];
    // x indices of the 4 entries at j .. j + 3.  Every load of the loop is unconditional -- a position past the row's end
    // (padding, or the look-ahead behind the last step) re-reads the row's last entry and is zeroed or dropped afterwards:
    // a load behind a per-element condition would be branched around and waited for one by one.
    auto columns = [&](int j, int32_t (&cn)[4], int (&cb)[4]) {   // column node and unknown of the entries j .. j + 3
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int jj = min(j + e, L - 1), k = jj / NV;
        cb[e] = jj - k * NV;
        cn[e] = bcol[b0 + k];
      }
    };
    int32_t cn[4], nn[4];
    int cb[4], nb[4];
    columns(4 * lane, cn, cb);
    for (int j = 4 * lane; j < Lp; j += 4 * F32_LANES) {
      // the next step's column nodes are requested together with this step's values and x entries and used a step later:
      // the bcol -> x chain then costs one memory latency per step, not two
      columns(j + 4 * F32_LANES, nn, nb);
      f32x4 v[NV];
#pragma unroll
      for (int a = 0; a < NV; a++) v[a] = __builtin_nontemporal_load((const f32x4*)(vrow + (int64_t)a * Lp + j));
      double xv[4];
#pragma unroll
      for (int e = 0; e < 4; e++) xv[e] = x[(int64_t)cn[e] * NV + cb[e]];
      __builtin_amdgcn_sched_barrier(0);   // keep the three groups of loads ahead of the arithmetic
#pragma unroll
      for (int e = 0; e < 4; e++) {
        xv[e] = j + e < L ? xv[e] : 0.0;
        cn[e] = nn[e];
        cb[e] = nb[e];
      }
#pragma unroll
      for (int a = 0; a < NV; a++) {
        acc[a] = fma((double)v[a].x, xv[0], acc[a]);
        acc[a] = fma((double)v[a].y, xv[1], acc[a]);
        acc[a] = fma((double)v[a].z, xv[2], acc[a]);
        acc[a] = fma((double)v[a].w, xv[3], acc[a]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int off = F32_LANES / 2; off >= 1; off >>= 1) acc[a] += __shfl_xor(acc[a], off, F32_LANES);
}

// one node on the FP64 values.  IDENT (level 0): the operator is D^-1 A, whose block diagonal is the identity, and dinv is the
// D^-1 of the operator (k_spmv, EPI 2); otherwise dinv is the D_l^-1 of the smoother (k_smooth)
template <int NV, bool IDENT>
__device__ __forceinline__ void gs_node(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                        const double* __restrict__ val, const double* __restrict__ dinv, const double* __restrict__ r,
                                        double* x, int64_t node, bool live, int lane) {
  double acc[NV];
  row_product<NV>(bptr, bcol, val, x, node, live, lane, acc);
  if (live && lane < NV) {
    const int64_t i = node * NV + lane;
    const double* __restrict__ drow = dinv + i * NV;
    double z = 0.0;
    if (IDENT) {
#pragma unroll
      for (int a = 0; a < NV; a++) z = fma(drow[a], acc[a], z);
      z = r[i] - z;
    } else {
#pragma unroll
      for (int q = 0; q < NV; q++) z = fma(drow[q], r[node * NV + q] - acc[q], z);
    }
    x[i] = x[i] + z;
  }
}

// one node on the fp32 copy of D^-1 A (level 0 of rdc_solve_mixed): no epilogue, the copy is scaled
template <int NV>
__device__ __forceinline__ void gs_node_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                            const int64_t* __restrict__ voff, const float* __restrict__ val32,
                                            const double* __restrict__ r, double* x, int64_t node, bool live, int lane) {
  double acc[NV];
  row_product_f32<NV>(bptr, bcol, voff, val32, x, node, live, lane, acc);
  double t = acc[0];
#pragma unroll
  for (int a = 1; a < NV; a++) t = lane == a ? acc[a] : t;
  if (live && lane < NV) {
    const int64_t i = node * NV + lane;
    x[i] = x[i] + (r[i] - t);
  }
}

// the nodes list[0 .. count) of one colour: 16 lanes per node as k_spmv
template <int NV, bool IDENT>
__global__ __launch_bounds__(256) void k_gs(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                            const double* __restrict__ val, const double* __restrict__ dinv,
                                            const double* __restrict__ r, double* x, const int32_t* __restrict__ list, int64_t count) {
  const int64_t at = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  const bool live = at < count;
  gs_node<NV, IDENT>(bptr, bcol, val, dinv, r, x, live ? list[at] : 0, live, threadIdx.x & 15);
}

// ... 8 lanes per node as k_spmv_f32
template <int NV>
__global__ __launch_bounds__(256) void k_gs_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                const int64_t* __restrict__ voff, const float* __restrict__ val32,
                                                const double* __restrict__ r, double* x, const int32_t* __restrict__ list, int64_t count) {
  const int64_t at = (int64_t)blockIdx.x * F32_NODES + (threadIdx.x / F32_LANES);
  const bool live = at < count;
  gs_node_f32<NV>(bptr, bcol, voff, val32, r, x, live ? list[at] : 0, live, threadIdx.x & (F32_LANES - 1));
}

// `sweeps` whole sweeps over a level of at most MG_GS_FUSED_NODES nodes in one workgroup: the colours in order, a barrier behind
// each (it also makes the stores to x visible to the other waves of the workgroup).  The trip counts are uniform over the
// lanes of a node and the barriers over the workgroup.
constexpr int GS_FUSED_THREADS = 1024;

template <int NV, bool IDENT>
__global__ __launch_bounds__(GS_FUSED_THREADS) void k_gs_fused(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                               const double* __restrict__ val, const double* __restrict__ dinv,
                                                               const double* __restrict__ r, double* x, const int32_t* __restrict__ list,
                                                               const int64_t* __restrict__ cptr, int n_colours, int sweeps) {
  for (int s = 0; s < sweeps; s++)
    for (int c = 0; c < n_colours; c++) {
      const int64_t c1 = cptr[c + 1];
      for (int64_t at0 = cptr[c]; at0 < c1; at0 += GS_FUSED_THREADS / 16) {
        const int64_t at = at0 + (threadIdx.x >> 4);
        const bool live = at < c1;
        gs_node<NV, IDENT>(bptr, bcol, val, dinv, r, x, live ? list[at] : 0, live, threadIdx.x & 15);
      }
      __syncthreads();
    }
}

template <int NV>
__global__ __launch_bounds__(GS_FUSED_THREADS) void k_gs_f32_fused(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                                   const int64_t* __restrict__ voff, const float* __restrict__ val32,
                                                                   const double* __restrict__ r, double* x, const int32_t* __restrict__ list,
                                                                   const int64_t* __restrict__ cptr, int n_colours, int sweeps) {
  for (int s = 0; s < sweeps; s++)
    for (int c = 0; c < n_colours; c++) {
      const int64_t c1 = cptr[c + 1];
      for (int64_t at0 = cptr[c]; at0 < c1; at0 += GS_FUSED_THREADS / F32_LANES) {
        const int64_t at = at0 + (threadIdx.x / F32_LANES);
        const bool live = at < c1;
        gs_node_f32<NV>(bptr, bcol, voff, val32, r, x, live ? list[at] : 0, live, threadIdx.x & (F32_LANES - 1));
      }
      __syncthreads();
    }
}

// Across ranks (RDC_PRECOND_MULTIGRID_GS_LOCAL, levels below the matrix): a sweep that is followed by the exchange of x fills the level's
// send buffer as k_smooth_pack does, from the register the lane stores to x.  The arithmetic is that of gs_node<NV, false>.
template <int NV>
__device__ __forceinline__ void gs_node_pack(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                             const double* __restrict__ val, const double* __restrict__ dinv, const double* __restrict__ r,
                                             double* x, int64_t node, bool live, int lane, const SendList& send) {
  double acc[NV];
  row_product<NV>(bptr, bcol, val, x, node, live, lane, acc);
  if (live && lane < NV) {
    const int64_t i = node * NV + lane;
    const double* __restrict__ drow = dinv + i * NV;
    double z = 0.0;
#pragma unroll
    for (int q = 0; q < NV; q++) z = fma(drow[q], r[node * NV + q] - acc[q], z);
    const double xn = x[i] + z;
    x[i] = xn;
    pack_entry<NV>(send, node, lane, xn);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void k_gs_pack(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                 const double* __restrict__ val, const double* __restrict__ dinv,
                                                 const double* __restrict__ r, double* x, const int32_t* __restrict__ list, int64_t count,
                                                 SendList send) {
  const int64_t at = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  const bool live = at < count;
  gs_node_pack<NV>(bptr, bcol, val, dinv, r, x, live ? list[at] : 0, live, threadIdx.x & 15, send);
}

// one whole sweep in one workgroup (the exchange stands between two sweeps, so a launch never holds more than one)
template <int NV>
__global__ __launch_bounds__(GS_FUSED_THREADS) void k_gs_fused_pack(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                                    const double* __restrict__ val, const double* __restrict__ dinv,
                                                                    const double* __restrict__ r, double* x, const int32_t* __restrict__ list,
                                                                    const int64_t* __restrict__ cptr, int n_colours, SendList send) {
  for (int c = 0; c < n_colours; c++) {
    const int64_t c1 = cptr[c + 1];
    for (int64_t at0 = cptr[c]; at0 < c1; at0 += GS_FUSED_THREADS / 16) {
      const int64_t at = at0 + (threadIdx.x >> 4);
      const bool live = at < c1;
      gs_node_pack<NV>(bptr, bcol, val, dinv, r, x, live ? list[at] : 0, live, threadIdx.x & 15, send);
    }
    __syncthreads();
  }
}

// ---- multicolour block ILU(0) (precond 4): M = (LU)^-1 from the right, LU the block ILU(0) of A^ = D^-1 A ----
//
// The factor lives in a copy of A^ in a layout of its own (rdc_solve.h, ilu_value_offset: per node the lower blocks in elimination
// order, the diagonal block, the upper blocks).  Nodes are eliminated by (colour, node id); no two nodes of a colour are coupled, so
// a colour is one launch: of the factorisation (k_ilu_factor), of the forward sweep (k_ilu_fwd) and of the backward sweep
// (k_ilu_bwd).  16 lanes per node throughout, as k_spmv.

// A^ = D^-1 A into the private layout: a lane takes the positions p = lane, lane + 16, ... of its node, finds the block of the same
// column in the CSR row (bcol ascends: binary search), reads it once (non-temporal) and multiplies it by D^-1 from the left
// (scaled_block: ascending, no contraction).  Runs after k_precond_setup.
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_copy(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                  const int32_t* __restrict__ pcol, const int32_t* __restrict__ nlow,
                                                  const double* __restrict__ val, const double* __restrict__ dinv, int64_t n_owned,
                                                  double* __restrict__ fval) {
  const int lane = threadIdx.x & 15;
  const int64_t node = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  if (node >= n_owned) return;
  const int64_t b0 = bptr[node], len = bptr[node + 1] - b0, nl = nlow[node];
  const double* __restrict__ vrow = val + (int64_t)NV * NV * b0;
  double di[NV][NV];
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int b = 0; b < NV; b++) di[a][b] = dinv[(node * NV + a) * NV + b];
  for (int64_t p = lane; p < len; p += 16) {
    const int32_t j = pcol[b0 + p];
    int64_t lo = 0, hi = len - 1, k = 0;
    while (lo <= hi) {   // the row has the column: pcol is a permutation of bcol within the node
      k = lo + (hi - lo) / 2;
      const int32_t c = bcol[b0 + k];
      if (c == j) break;
      if (c < j) lo = k + 1; else hi = k - 1;
    }
    double blk[NV][NV], out[NV][NV];
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) blk[a][b] = __builtin_nontemporal_load(vrow + ((int64_t)a * len + k) * NV + b);
    scaled_block<NV>(di, blk, out);
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) fval[ilu_value_offset(b0, NV, len, nl, a, p, b)] = out[a][b];
  }
}

// k_ilu_copy on lists with ghost columns (rdc_solve.h): the node's owned positions only, own = nown[node] of them.  Its owned
// columns are the first `own` of its CSR row (ghost ids lie above every owned id and bcol ascends), so the search stays among them
// and neither the column nor the values of a ghost block are read; the CSR rows keep their stride of len blocks.  A kernel of its
// own text and no instantiation of a shared body: through one k_ilu_copy compiles to other (equivalent) instructions than it did.
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_copy_owned(const int64_t* __restrict__ bptr, const int32_t* __restrict__ bcol,
                                                        const int32_t* __restrict__ pcol, const int32_t* __restrict__ nlow,
                                                        const int32_t* __restrict__ nown, const double* __restrict__ val,
                                                        const double* __restrict__ dinv, int64_t n_owned, double* __restrict__ fval) {
  const int lane = threadIdx.x & 15;
  const int64_t node = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  if (node >= n_owned) return;
  const int64_t b0 = bptr[node], len = bptr[node + 1] - b0, nl = nlow[node], own = nown[node];
  const double* __restrict__ vrow = val + (int64_t)NV * NV * b0;
  double di[NV][NV];
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int b = 0; b < NV; b++) di[a][b] = dinv[(node * NV + a) * NV + b];
  for (int64_t p = lane; p < own; p += 16) {
    const int32_t j = pcol[b0 + p];
    int64_t lo = 0, hi = own - 1, k = 0;
    while (lo <= hi) {   // the owned part of the row has the column
      k = lo + (hi - lo) / 2;
      const int32_t c = bcol[b0 + k];
      if (c == j) break;
      if (c < j) lo = k + 1; else hi = k - 1;
    }
    double blk[NV][NV], out[NV][NV];
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) blk[a][b] = __builtin_nontemporal_load(vrow + ((int64_t)a * len + k) * NV + b);
    scaled_block<NV>(di, blk, out);
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) fval[ilu_value_offset(b0, NV, own, nl, a, p, b)] = out[a][b];
  }
}

// The nodes list[0 .. count) of one colour, one 16-lane group each (rdc_solve.h, ilu_factor_node: the lanes run over the upper
// blocks of the row of a lower neighbour, whose targets in the node's own row are distinct).  The row is read and written in
// global memory whatever its length; between two lower neighbours a workgroup-scope fence makes the blocks the 16 lanes have
// just written visible to all of them (they are lanes of one wave, so they reach it together).  fval and uinv are read (rows and
// pivots of lower colours, final since an earlier launch) and written (the node's own): neither const nor __restrict__.
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_factor(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                    const int32_t* __restrict__ nlow, const int32_t* __restrict__ colour, double* fval,
                                                    double* uinv, const int32_t* __restrict__ list, int64_t count,
                                                    SolveScal* __restrict__ scal) {
  const int64_t at = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  if (at >= count) return;
  const bool ok = ilu_factor_node<NV>(bptr, pcol, nlow, colour, fval, uinv, list[at], threadIdx.x & 15, 16,
                                      [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); });
  if (!ok) atomicAdd(&scal->bad_blocks, 1);
}

// ... on lists with ghost columns: the rows of the node and of its lower neighbours end at their owned positions (nown), and
// ilu_find searches the owned part of the node's row only -- `colour` has no entry for a ghost
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_factor_owned(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                          const int32_t* __restrict__ nlow, const int32_t* __restrict__ nown,
                                                          const int32_t* __restrict__ colour, double* fval, double* uinv,
                                                          const int32_t* __restrict__ list, int64_t count, SolveScal* __restrict__ scal) {
  const int64_t at = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  if (at >= count) return;
  const bool ok = ilu_factor_node<NV, true>(bptr, pcol, nlow, colour, fval, uinv, list[at], threadIdx.x & 15, 16,
                                            [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }, nown);
  if (!ok) atomicAdd(&scal->bad_blocks, 1);
}

// acc[a] = sum over the run `vrow` (NV rows of L entries: the lower or the upper blocks of a node, columns cols[0 .. L / NV)) of
// value times x, in all 16 lanes: row_product on a run of the private layout
template <int NV>
__device__ __forceinline__ void ilu_run_product(const double* __restrict__ vrow, int L, const int32_t* __restrict__ cols, const double* x,
                                                int lane, double (&acc)[NV]) {
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  for (int j = lane; j < L; j += 16) {
    const int k = j / NV, b = j - k * NV;
    const double xv = x[(int64_t)cols[k] * NV + b];
#pragma unroll
    for (int a = 0; a < NV; a++) acc[a] = fma(__builtin_nontemporal_load(vrow + (int64_t)a * L + j), xv, acc[a]);
  }
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) acc[a] += __shfl_xor(acc[a], off, 16);
}

// forward sweep over one colour: z_i = y_i - sum_{colour(k) < c} L_ik z_k.  z is read (lower colours) and written (this one);
// y is the argument of the apply and does not overlap z.  Colour 0 has no lower blocks: its launch copies y.
// Serves lists with ghost columns as it is: the lower run starts at nvar^2 * bptr[node] and has nlow[node] blocks whatever follows
// it, and a lower column has a lower colour, so it is an owned node: z is read below n_owned only.
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_fwd(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                 const int32_t* __restrict__ nlow, const double* __restrict__ fval,
                                                 const double* __restrict__ y, double* z, const int32_t* __restrict__ list, int64_t count) {
  const int lane = threadIdx.x & 15;
  const int64_t at = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  const bool live = at < count;
  const int64_t node = live ? list[at] : 0;
  const int64_t b0 = bptr[node];
  double acc[NV];
  ilu_run_product<NV>(fval + (int64_t)NV * NV * b0, live ? nlow[node] * NV : 0, pcol + b0, z, lane, acc);
  double t = acc[0];
#pragma unroll
  for (int a = 1; a < NV; a++) t = lane == a ? acc[a] : t;
  if (live && lane < NV) z[node * NV + lane] = y[node * NV + lane] - t;
}

// backward sweep over one colour: z_i = U_ii^-1 (z_i - sum_{colour(j) > c} U_ij z_j), in place
// OWNED (lists with ghost columns): the upper run ends at the node's owned positions, so z is read below n_owned only
template <int NV, bool OWNED>
__device__ __forceinline__ void ilu_bwd_body(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                             const int32_t* __restrict__ nlow, const int32_t* __restrict__ nown,
                                             const double* __restrict__ fval, const double* __restrict__ uinv, double* z,
                                             const int32_t* __restrict__ list, int64_t count) {
  const int lane = threadIdx.x & 15;
  const int64_t at = (int64_t)blockIdx.x * SPMV_NODES + (threadIdx.x >> 4);
  const bool live = at < count;
  const int64_t node = live ? list[at] : 0;
  const int64_t b0 = bptr[node], len = OWNED ? (int64_t)nown[node] : bptr[node + 1] - b0, nl = nlow[node];
  double acc[NV];
  ilu_run_product<NV>(fval + (int64_t)NV * NV * (b0 + nl + 1), live ? (int)(len - nl - 1) * NV : 0, pcol + b0 + nl + 1, z, lane, acc);
  if (live && lane < NV) {
    const double* __restrict__ urow = uinv + (node * NV + lane) * NV;
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < NV; q++) t = fma(urow[q], z[node * NV + q] - acc[q], t);
    z[node * NV + lane] = t;
  }
}

template <int NV>
__global__ __launch_bounds__(256) void k_ilu_bwd(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                 const int32_t* __restrict__ nlow, const double* __restrict__ fval,
                                                 const double* __restrict__ uinv, double* z, const int32_t* __restrict__ list, int64_t count) {
  ilu_bwd_body<NV, false>(bptr, pcol, nlow, nullptr, fval, uinv, z, list, count);
}

template <int NV>
__global__ __launch_bounds__(256) void k_ilu_bwd_owned(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                       const int32_t* __restrict__ nlow, const int32_t* __restrict__ nown,
                                                       const double* __restrict__ fval, const double* __restrict__ uinv, double* z,
                                                       const int32_t* __restrict__ list, int64_t count) {
  ilu_bwd_body<NV, true>(bptr, pcol, nlow, nown, fval, uinv, z, list, count);
}

// ---- the fp32 copy of the factor (option "ilu_factor_bits" = 32; layout: rdc_solve.h, ilu_f32_offset) ----
//
// The factorisation stays what it is; k_ilu_round_f32 rounds its lower and upper blocks into the copy, and the sweeps below stream
// that instead of the FP64 runs: 8 lanes per node and 16-byte loads as k_spmv_f32, every value converted to double and fed to an
// fma, so z, the sums and the U_ii^-1 epilogue are FP64.  A lane adds its own entries in ascending order, then a fixed butterfly.

// The copy of every owned node from the factor: a lane takes the positions p = lane, lane + 8, ... of the node's runs (nown: its
// owned positions, on lists with ghost columns; null: the whole row), skips the diagonal block, and stores the zero padding of
// the rows of both runs.  Counts the entries that are finite in FP64 and not in fp32: the sweeps then stay with the FP64 factor.
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_round_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ nlow,
                                                       const int32_t* __restrict__ nown, const double* __restrict__ fval,
                                                       const int64_t* __restrict__ foff, int64_t n_owned, float* __restrict__ val32,
                                                       SolveScal* __restrict__ scal) {
  const int lane = threadIdx.x & (F32_LANES - 1);
  const int64_t node = (int64_t)blockIdx.x * F32_NODES + (threadIdx.x / F32_LANES);
  if (node >= n_owned) return;
  const int64_t b0 = bptr[node], len = nown ? (int64_t)nown[node] : bptr[node + 1] - b0, nl = nlow[node], f0 = foff[node];
  int bad = 0;
  for (int64_t p = lane; p < len; p += F32_LANES) {
    if (p == nl) continue;
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) {
        const double v = fval[ilu_value_offset(b0, NV, len, nl, a, p, b)];
        const float f = (float)v;
        bad += finite_d(v) && !solve_finite_f32(f);
        val32[ilu_f32_offset(f0, NV, len, nl, a, p, b)] = f;
      }
  }
  const int64_t nup = len - nl - 1;
  const int64_t sl = f32_row_stride(NV, nl), su = f32_row_stride(NV, nup);
  if (lane < sl - nl * NV)   // at most 3 padding floats per row
#pragma unroll
    for (int a = 0; a < NV; a++) val32[f0 + a * sl + nl * NV + lane] = 0.0f;
  if (lane < su - nup * NV)
#pragma unroll
    for (int a = 0; a < NV; a++) val32[f0 + NV * sl + a * su + nup * NV + lane] = 0.0f;
  if (bad) atomicAdd(&scal->ilu_overflow, bad);
}

// ilu_run_product on a run of the fp32 copy, in all 8 lanes: vrow holds NV rows of stride f32_row_stride(NV, blocks), L = blocks *
// NV of them entries.  The loop is that of k_spmv_f32: every load is unconditional, a position past the run's end re-reads the
// run's last column and is zeroed afterwards, and the next step's columns are requested a step ahead.
template <int NV>
__device__ __forceinline__ void ilu_run_product_f32(const float* __restrict__ vrow, int L, const int32_t* __restrict__ cols, const double* x,
                                                    int lane, double (&acc)[NV]) {
#pragma unroll
  for (int a = 0; a < NV; a++) acc[a] = 0.0;
  if (L > 0) {
    const int Lp = (L + 3) & ~3;
    auto columns = [&](int j, int32_t (&cn)[4], int (&cb)[4]) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int jj = min(j + e, L - 1), k = jj / NV;
        cb[e] = jj - k * NV;
        cn[e] = cols[k];
      }
    };
    int32_t cn[4], nn[4];
    int cb[4], nb[4];
    columns(4 * lane, cn, cb);
    for (int j = 4 * lane; j < Lp; j += 4 * F32_LANES) {
      columns(j + 4 * F32_LANES, nn, nb);
      f32x4 v[NV];
#pragma unroll
      for (int a = 0; a < NV; a++) v[a] = __builtin_nontemporal_load((const f32x4*)(vrow + (int64_t)a * Lp + j));
      double xv[4];
#pragma unroll
      for (int e = 0; e < 4; e++) xv[e] = x[(int64_t)cn[e] * NV + cb[e]];
      __builtin_amdgcn_sched_barrier(0);   // keep the three groups of loads ahead of the arithmetic
#pragma unroll
      for (int e = 0; e < 4; e++) {
        xv[e] = j + e < L ? xv[e] : 0.0;
        cn[e] = nn[e];
        cb[e] = nb[e];
      }
#pragma unroll
      for (int a = 0; a < NV; a++) {
        acc[a] = fma((double)v[a].x, xv[0], acc[a]);
        acc[a] = fma((double)v[a].y, xv[1], acc[a]);
        acc[a] = fma((double)v[a].z, xv[2], acc[a]);
        acc[a] = fma((double)v[a].w, xv[3], acc[a]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NV; a++)
#pragma unroll
    for (int off = F32_LANES / 2; off >= 1; off >>= 1) acc[a] += __shfl_xor(acc[a], off, F32_LANES);
}

// k_ilu_fwd on the fp32 copy (serves lists with ghost columns as it is: the lower run is the node's first, whatever follows)
template <int NV>
__global__ __launch_bounds__(256) void k_ilu_fwd_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                     const int32_t* __restrict__ nlow, const int64_t* __restrict__ foff,
                                                     const float* __restrict__ val32, const double* __restrict__ y, double* z,
                                                     const int32_t* __restrict__ list, int64_t count) {
  const int lane = threadIdx.x & (F32_LANES - 1);
  const int64_t at = (int64_t)blockIdx.x * F32_NODES + (threadIdx.x / F32_LANES);
  const bool live = at < count;
  const int64_t node = live ? list[at] : 0;
  double acc[NV];
  ilu_run_product_f32<NV>(val32 + foff[node], live ? nlow[node] * NV : 0, pcol + bptr[node], z, lane, acc);
  double t = acc[0];
#pragma unroll
  for (int a = 1; a < NV; a++) t = lane == a ? acc[a] : t;
  if (live && lane < NV) z[node * NV + lane] = y[node * NV + lane] - t;
}

// ilu_bwd_body on the fp32 copy: the upper run lies behind the NV padded rows of the lower one; U_ii^-1 is the FP64 array
template <int NV, bool OWNED>
__device__ __forceinline__ void ilu_bwd_f32_body(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                 const int32_t* __restrict__ nlow, const int32_t* __restrict__ nown,
                                                 const int64_t* __restrict__ foff, const float* __restrict__ val32,
                                                 const double* __restrict__ uinv, double* z, const int32_t* __restrict__ list,
                                                 int64_t count) {
  const int lane = threadIdx.x & (F32_LANES - 1);
  const int64_t at = (int64_t)blockIdx.x * F32_NODES + (threadIdx.x / F32_LANES);
  const bool live = at < count;
  const int64_t node = live ? list[at] : 0;
  const int64_t b0 = bptr[node], len = OWNED ? (int64_t)nown[node] : bptr[node + 1] - b0, nl = nlow[node];
  double acc[NV];
  ilu_run_product_f32<NV>(val32 + foff[node] + NV * f32_row_stride(NV, nl), live ? (int)(len - nl - 1) * NV : 0, pcol + b0 + nl + 1, z, lane,
                          acc);
  if (live && lane < NV) {
    const double* __restrict__ urow = uinv + (node * NV + lane) * NV;
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < NV; q++) t = fma(urow[q], z[node * NV + q] - acc[q], t);
    z[node * NV + lane] = t;
  }
}

template <int NV>
__global__ __launch_bounds__(256) void k_ilu_bwd_f32(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                     const int32_t* __restrict__ nlow, const int64_t* __restrict__ foff,
                                                     const float* __restrict__ val32, const double* __restrict__ uinv, double* z,
                                                     const int32_t* __restrict__ list, int64_t count) {
  ilu_bwd_f32_body<NV, false>(bptr, pcol, nlow, nullptr, foff, val32, uinv, z, list, count);
}

template <int NV>
__global__ __launch_bounds__(256) void k_ilu_bwd_f32_owned(const int64_t* __restrict__ bptr, const int32_t* __restrict__ pcol,
                                                           const int32_t* __restrict__ nlow, const int32_t* __restrict__ nown,
                                                           const int64_t* __restrict__ foff, const float* __restrict__ val32,
                                                           const double* __restrict__ uinv, double* z, const int32_t* __restrict__ list,
                                                           int64_t count) {
  ilu_bwd_f32_body<NV, true>(bptr, pcol, nlow, nown, foff, val32, uinv, z, list, count);
}

// First use of every kernel instantiation. A code object lists template instantiations by first use; this list keeps the order
// they have had since each was added, whatever order the launch code below uses them in, so that the device assembly of two
// revisions can be compared byte for byte.
#define KERNELS_OF(NV)                                                                                                          \
  (const void*)k_galerkin<NV, true>, (const void*)k_galerkin<NV, false>, (const void*)k_residual<NV>,                            \
  (const void*)k_smooth<NV, true, true>, (const void*)k_spmv<NV, 2>, (const void*)k_restrict<NV>,                                \
  (const void*)k_smooth<NV, true, false>, (const void*)k_smooth<NV, false, false>, (const void*)k_prolong<NV>
#define GS_KERNELS_OF(NV)                                                                                                       \
  (const void*)k_gs<NV, true>, (const void*)k_gs<NV, false>, (const void*)k_gs_f32<NV>, (const void*)k_gs_fused<NV, true>,     \
  (const void*)k_gs_fused<NV, false>, (const void*)k_gs_f32_fused<NV>
#define ILU_KERNELS_OF(NV) (const void*)k_ilu_copy<NV>, (const void*)k_ilu_factor<NV>, (const void*)k_ilu_fwd<NV>, (const void*)k_ilu_bwd<NV>
#define ILU_OWNED_KERNELS_OF(NV) (const void*)k_ilu_copy_owned<NV>, (const void*)k_ilu_factor_owned<NV>, (const void*)k_ilu_bwd_owned<NV>
#define ILU_F32_KERNELS_OF(NV)                                                                                                  \
  (const void*)k_ilu_round_f32<NV>, (const void*)k_ilu_fwd_f32<NV>, (const void*)k_ilu_bwd_f32<NV>, (const void*)k_ilu_bwd_f32_owned<NV>
[[maybe_unused]] const void* const KERNEL_ORDER[] = {
    (const void*)k_spmv<3, 1>, (const void*)k_spmv<3, 0>, (const void*)k_spmv<5, 1>, (const void*)k_spmv<5, 0>,
    (const void*)k_spmv_f32<3, 1>, (const void*)k_spmv_f32<3, 0>, (const void*)k_spmv_f32<5, 1>, (const void*)k_spmv_f32<5, 0>,
    (const void*)k_precond_setup<3>, (const void*)k_scale_f32<3>, (const void*)k_precond_setup<5>, (const void*)k_scale_f32<5>,
    KERNELS_OF(3), (const void*)k_update_xr<true>, (const void*)k_update_xr<false>, KERNELS_OF(5),
    (const void*)k_reduce, (const void*)k_advance, (const void*)k_halo_pack<3>, (const void*)k_halo_pack<5>,
    (const void*)k_restrict_pack<3>, (const void*)k_prolong_pack<3>, (const void*)k_smooth_pack<3>,
    (const void*)k_restrict_pack<5>, (const void*)k_prolong_pack<5>, (const void*)k_smooth_pack<5>,
    GS_KERNELS_OF(3), GS_KERNELS_OF(5), ILU_KERNELS_OF(3), ILU_KERNELS_OF(5), ILU_OWNED_KERNELS_OF(3), ILU_OWNED_KERNELS_OF(5),
    ILU_F32_KERNELS_OF(3), ILU_F32_KERNELS_OF(5),
    (const void*)k_gs_pack<3>, (const void*)k_gs_fused_pack<3>, (const void*)k_gs_pack<5>, (const void*)k_gs_fused_pack<5>};
#undef KERNELS_OF
#undef GS_KERNELS_OF
#undef ILU_KERNELS_OF
#undef ILU_OWNED_KERNELS_OF
#undef ILU_F32_KERNELS_OF

// ---- restarted GMRES(m) (option "solve_method" = 1): classical Gram-Schmidt on the basis V, one launch for all
// inner products of a step and one for the update.  State and layout: GmresState (rdc_solve.h).  Every sum has a fixed order
// (a thread's own entries ascending, the wave butterfly, the four waves in order, the workgroups through k_gmres_finalize): no
// floating-point atomics, no dependence on the launch shape, two solves bitwise equal. ----

enum { GMRES_STAGE_DOTS = 0, GMRES_STAGE_DOTS2 = 1, GMRES_STAGE_NORM = 2, GMRES_STAGE_START = 3 };

// (v_k, w) for k < nbasis and (w, w), one launch: a workgroup keeps its VEC_PER_BLOCK chunk of w in registers and streams the
// matching chunk of every basis vector once.  Partials component-major: component k of this workgroup at partials[k * nparts + block].
__global__ __launch_bounds__(256) void k_gmres_dots(const double* __restrict__ V, int64_t stride, int nbasis, const double* __restrict__ w,
                                                    int64_t n, double* __restrict__ partials, int64_t nparts) {
  __shared__ double sh[GMRES_MAX_RESTART + 1][4];
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
  double wv[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    wv[q] = i < n ? __builtin_nontemporal_load(w + i) : 0.0;
  }
  const int wave = threadIdx.x >> 6;
  for (int k = 0; k <= nbasis; k++) {
    double s = 0.0;
    if (k < nbasis) {
      const double* __restrict__ vk = V + (int64_t)k * stride;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t i = i0 + q * 256;
        if (i < n) s = fma(__builtin_nontemporal_load(vk + i), wv[q], s);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) s = fma(wv[q], wv[q], s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) sh[k][wave] = s;
  }
  __syncthreads();
  for (int k = threadIdx.x; k <= nbasis; k += 256) partials[(int64_t)k * nparts + blockIdx.x] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
}

// w -= sum_k h_k v_k (k < nbasis, ascending), in place in the slot of w, with the partials of ||w||^2 (component 0).  Reads w once
// and every v_k once.  A flagged step (an inner product was not finite) leaves w alone.
__global__ __launch_bounds__(256) void k_gmres_orth(const double* __restrict__ V, int64_t stride, int nbasis, double* __restrict__ w,
                                                    int64_t n, const double* __restrict__ h, double* __restrict__ partials,
                                                    const GmresRec* __restrict__ rec) {
  if (rec->flag & GMRES_NOT_FINITE) return;   // uniform
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
  double wv[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    wv[q] = i < n ? __builtin_nontemporal_load(w + i) : 0.0;
  }
  for (int k = 0; k < nbasis; k++) {
    const double hk = h[k];
    const double* __restrict__ vk = V + (int64_t)k * stride;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t i = i0 + q * 256;
      if (i < n) wv[q] = fma(-hk, __builtin_nontemporal_load(vk + i), wv[q]);
    }
  }
  double c[1] = {0.0};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) {
      w[i] = wv[q];
      c[0] = fma(wv[q], wv[q], c[0]);
    }
  }
  block_partials<1>(c, partials);
}

// The sums of `ncomp` components of component-major partials in a fixed order (one workgroup of 1024), four components at a time,
// into tot (shared memory; valid for every thread on return).
__device__ __forceinline__ void gmres_sum_partials(const double* __restrict__ partials, int64_t nparts, int ncomp, double (&sh)[4][1024],
                                                   double* tot) {
  for (int c0 = 0; c0 < ncomp; c0 += 4) {
    const int nc = min(4, ncomp - c0);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nparts; i += 1024)
      for (int c = 0; c < nc; c++) s[c] += partials[(int64_t)(c0 + c) * nparts + i];
    for (int c = 0; c < 4; c++) sh[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off)
        for (int c = 0; c < nc; c++) sh[c][threadIdx.x] += sh[c][threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0)
      for (int c = 0; c < nc; c++) tot[c0 + c] = sh[c][0];
    __syncthreads();
  }
}

// a flagged step wrote no partials: the stages behind its first sum have nothing to add up
__device__ __forceinline__ bool gmres_stage_skipped(int stage, const GmresRec* rec) {
  return stage != GMRES_STAGE_DOTS && stage != GMRES_STAGE_START && (rec->flag & GMRES_NOT_FINITE);
}

// What a step does with its sums (one thread).  DOTS: h_{0..j,j} of the first Gram-Schmidt pass and (w, w); DOTS2: the second pass,
// added to the first; NORM: h_{j+1,j} = ||w||, the Givens step of column j in device memory, and the record; START (the hook):
// beta^2.  tot: the sums, of this partition or, across ranks, of all of them -- the same bits in give the same bits out.
__device__ __forceinline__ void gmres_advance(const double* tot, int stage, int j, const GmresState& G) {
  GmresRec* rec = G.rec;
  const int ld = G.restart + 1;
  double* hcol = G.H + (int64_t)j * ld;
  if (stage == GMRES_STAGE_START) {
    G.scal[0] = tot[0];
  } else if (stage == GMRES_STAGE_DOTS || stage == GMRES_STAGE_DOTS2) {
    bool ok = true;
    for (int k = 0; k <= j; k++) {
      const double hk = stage == GMRES_STAGE_DOTS ? tot[k] : hcol[k] + tot[k];
      G.hpass[k] = tot[k];
      hcol[k] = hk;
      ok = ok && finite_d(tot[k]) && finite_d(hk);
    }
    ok = ok && finite_d(tot[j + 1]);
    if (stage == GMRES_STAGE_DOTS) {
      rec->wn2 = tot[j + 1];
      rec->flag = ok ? 0 : GMRES_NOT_FINITE;
    } else if (!ok) {
      rec->flag |= GMRES_NOT_FINITE;
    }
  } else {
    const double hn = sqrt(tot[0]);
    hcol[j + 1] = hn;
    rec->hnext = hn;
    const int f = gmres_givens_step(j, hcol, G.R + (int64_t)j * ld, G.cs, G.sn, G.g);
    if (f) {
      rec->flag |= f;
      return;
    }
    rec->est = fabs(G.g[j + 1]);
    if (hn == 0.0) rec->flag |= GMRES_HAPPY;
    else G.scal[1] = 1.0 / hn;
  }
}

// The sums of a step's partials and what the step does with them, in one launch: the single-partition form.
__global__ __launch_bounds__(1024) void k_gmres_finalize(const double* __restrict__ partials, int64_t nparts, int ncomp, int stage, int j,
                                                         GmresState G) {
  __shared__ double sh[4][1024];
  __shared__ double tot[GMRES_MAX_RESTART + 1];
  if (gmres_stage_skipped(stage, G.rec)) {
    if (threadIdx.x == 0 && stage == GMRES_STAGE_NORM) G.rec->hnext = 0.0;
    return;
  }
  gmres_sum_partials(partials, nparts, ncomp, sh, tot);
  if (threadIdx.x != 0) return;
  gmres_advance(tot, stage, j, G);
}

// Across ranks: k_gmres_finalize in two halves with the wide all-reduce between them.  k_gmres_reduce: this rank's sums, in the same
// fixed order, into G.red[0 .. ncomp).  A skipped stage (the flag is the same on every rank) sends zeros.
__global__ __launch_bounds__(1024) void k_gmres_reduce(const double* __restrict__ partials, int64_t nparts, int ncomp, int stage, GmresState G) {
  __shared__ double sh[4][1024];
  __shared__ double tot[GMRES_MAX_RESTART + 1];
  const bool skip = gmres_stage_skipped(stage, G.rec);
  if (!skip) gmres_sum_partials(partials, nparts, ncomp, sh, tot);
  for (int k = threadIdx.x; k < ncomp; k += 1024) G.red[k] = skip ? 0.0 : tot[k];
}

// k_gmres_advance: the scalar work of the step on the all-reduced sums (one thread).  Every rank computes the same bits from the
// same bits: the estimate, the flags and, later, y are global, and every branch the host takes on the record is collective.
__global__ void k_gmres_advance(int stage, int j, GmresState G) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (gmres_stage_skipped(stage, G.rec)) {
    if (stage == GMRES_STAGE_NORM) G.rec->hnext = 0.0;
    return;
  }
  gmres_advance(G.red, stage, j, G);
}

// v_0 = src / beta with beta^2 in device memory (the ||r||^2 of k_residual, or the START sum of the hook); g = beta e_0 and a clean
// record.  beta = 0 or not finite: flagged, and v_0 is not written.
__global__ __launch_bounds__(256) void k_gmres_start(const double* __restrict__ src, const double* __restrict__ beta2, double* __restrict__ v0,
                                                     int64_t n, GmresState G) {
  const double beta = sqrt(*beta2);
  const bool ok = finite_d(beta) && beta > 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    G.g[0] = beta;
    G.scal[2] = 1.0;
    G.rec->est = beta; G.rec->hnext = 0.0; G.rec->wn2 = 0.0;
    G.rec->flag = ok ? 0 : GMRES_NOT_FINITE;
    G.rec->overflow = 0;
  }
  if (!ok) return;
  const double inv = 1.0 / beta;
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) v0[i] = src[i] * inv;
  }
}

// v_{j+1} = w / h_{j+1,j}, in place, the factor from device memory; a flagged step (not finite, or h_{j+1,j} = 0) leaves w alone
__global__ __launch_bounds__(256) void k_gmres_scale(double* __restrict__ w, int64_t n, const double* __restrict__ inv,
                                                     const GmresRec* __restrict__ rec) {
  if (rec->flag) return;   // uniform
  const double s = *inv;
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) w[i] = __builtin_nontemporal_load(w + i) * s;
  }
}

// y = R^-1 g for the leading k columns (one thread: k <= 128)
__global__ void k_gmres_solve_y(int k, GmresState G) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!gmres_back_substitute(G.restart + 1, k, G.R, G.g, G.y)) G.rec->flag |= GMRES_Y_NOT_FINITE;
}

// u = sum_k y_k v_k (k < K, ascending), or, ADD, x += that sum.  An entry of x whose update would not be finite keeps its value and
// is counted (an integer counter), as k_update_xr does it.  A y that is not finite: nothing is written.
template <bool ADD>
__global__ __launch_bounds__(256) void k_gmres_combine(const double* __restrict__ V, int64_t stride, int K, const double* __restrict__ y,
                                                       double* __restrict__ out, int64_t n, GmresRec* __restrict__ rec) {
  if (rec->flag & GMRES_Y_NOT_FINITE) return;   // uniform
  const int64_t i0 = (int64_t)blockIdx.x * VEC_PER_BLOCK + threadIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < K; k++) {
    const double yk = y[k];
    const double* __restrict__ vk = V + (int64_t)k * stride;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int64_t i = i0 + q * 256;
      if (i < n) s[q] = fma(yk, __builtin_nontemporal_load(vk + i), s[q]);
    }
  }
  int bad = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) {
      if (ADD) {
        const double xn = out[i] + s[q];
        if (finite_d(xn)) out[i] = xn;
        else bad++;
      } else {
        out[i] = s[q];
      }
    }
  }
  if (ADD && bad) atomicAdd(&rec->overflow, bad);
}

// ---- host side.  Launch shapes: the formulas of rdc_solve.h (op_blocks, op_parts, vec_blocks) and per_thread ----
dim3 per_thread(int64_t items) { return dim3((unsigned)cdiv(items, 256)); }                                   // one thread per item

#define SOLVE_HIP(call)                 \
  do {                                  \
    const hipError_t e_ = (call);       \
    if (e_ != hipSuccess) return e_;    \
  } while (0)

// f(std::integral_constant<int, nvar>) for the unknowns per node the kernels are instantiated for
template <class F>
hipError_t by_nvar(int nvar, F&& f) {
  if (nvar == 3) return f(std::integral_constant<int, 3>());
  if (nvar == 5) return f(std::integral_constant<int, 5>());
  return hipErrorInvalidValue;
}

// device time, in *ms, of what body() enqueues on the stream; returns behind it
template <class F>
hipError_t timed(hipStream_t stream, float* ms, F&& body) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  SOLVE_HIP(hipEventCreate(&e0));
  hipError_t e = hipEventCreate(&e1);
  if (e == hipSuccess) e = hipEventRecord(e0, stream);
  if (e == hipSuccess) e = body();
  if (e == hipSuccess) e = hipEventRecord(e1, stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
  (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return e;
}

// (the work buffer of a solve and its layout: Work, carve in rdc_solve.h)

// a callback's return: non-zero ends the solve, and nothing is called after it
hipError_t callback(const SolveDev& d, int rc) {
  if (rc == 0) return hipSuccess;
  *d.comm_rc = rc;
  return SOLVE_COMM_FAILED;
}

// y = A_l x on level l of the hierarchy, the one entry to the three SpMV kernels.  Level 0 is the context's matrix in the form
// asked for; a level below owns one matrix (PLAIN whatever `form` says).  dot_with: also the partials of (y, dot_with) and
// (y, y) (SCALED and F32 only).  PLAIN and F32 without a dot product need no Work.
// n0, n1: the rows of the nodes [n0, n1) only (level 0; n1 < 0: all).  The kernels see the node n0 as their node 0: whatever they
// index by node (bptr, voff, y, D^-1, dot_with) is shifted, whatever they reach through bptr and bcol (values, x) is not, since
// bptr and voff hold absolute offsets.  The partials of a range lie behind those of the rows [0, n0) (op_parts).
template <int NV>
hipError_t apply(const SolveDev& d, const Work* w, int l, Form form, const double* x, double* y, const double* dot_with,
                 int64_t n0 = 0, int64_t n1 = -1) {
  const MgLevelDev* L = l ? &d.mg->lv[l] : nullptr;
  if (L) form = PLAIN;
  if (form == PLAIN && dot_with) return hipErrorInvalidValue;
  if (n1 < 0) n1 = L ? L->n : d.n_owned;
  if (L && n0) return hipErrorInvalidValue;
  const int64_t n = n1 - n0;
  const dim3 grid((unsigned)op_blocks(n, form)), block(256);
  if (!grid.x) return hipSuccess;
  double* partials = dot_with ? w->partials + 2 * op_blocks(n0, form) : nullptr;
  y += n0 * NV;
  if (dot_with) dot_with += n0 * NV;
  if (form == F32) {
    hipLaunchKernelGGL((dot_with ? k_spmv_f32<NV, 1> : k_spmv_f32<NV, 0>), grid, block, 0, d.stream, d.bptr + n0, d.bcol, d.voff + n0,
                       (const float*)d.val32, x, y, n, dot_with, partials);
  } else {
    hipLaunchKernelGGL((form == PLAIN ? k_spmv<NV, 0> : dot_with ? k_spmv<NV, 1> : k_spmv<NV, 2>), grid, block, 0, d.stream,
                       (L ? L->bptr : d.bptr) + n0, L ? L->bcol : d.bcol, L ? (const double*)L->val : d.val, x, y, n,
                       form == PLAIN ? (const double*)nullptr : (const double*)w->dinv + n0 * NV * NV, dot_with, partials);
  }
  return hipGetLastError();
}

// y = A x on level 0 of a vector whose ghost entries the peers own: pack and exchange_begin, the rows that read no ghost,
// exchange_end, the other rows.  x is written: its ghost tail [n_owned, n_nodes) receives.  Without a communicator: apply.
template <int NV>
hipError_t apply_halo(const SolveDev& d, const Work& w, Form form, double* x, double* y, const double* dot_with) {
  if (!d.comm) return apply<NV>(d, &w, 0, form, x, y, dot_with);
  if (d.dist.n_send) {
    hipLaunchKernelGGL((k_halo_pack<NV>), per_thread(d.dist.n_send * NV), dim3(256), 0, d.stream, d.send_nodes, d.dist.n_send,
                       (const double*)x, w.send);
    SOLVE_HIP(hipGetLastError());
  }
  SOLVE_HIP(callback(d, d.comm->exchange_begin(d.comm->user, w.send, x + d.n_owned * NV, (void*)d.stream)));
  SOLVE_HIP(apply<NV>(d, &w, 0, form, x, y, dot_with, 0, d.dist.n_int));
  SOLVE_HIP(callback(d, d.comm->exchange_end(d.comm->user, (void*)d.stream)));
  return apply<NV>(d, &w, 0, form, x, y, dot_with, d.dist.n_int, d.n_owned);
}

// the scalars of a stage from the partials of the kernel before it.  With a communicator the sums cross the partitions on their
// way (k_reduce, allreduce_sum, k_advance); counters: the record also carries bad_blocks and f32_overflow (first residual).
// extra (with a communicator only): a rank-local int32 counter that rides in the record as its fifth value and comes back global.
hipError_t finalize(const SolveDev& d, const Work& w, int64_t nparts, int ncomp, int stage, bool counters = false, int32_t* extra = nullptr) {
  if (!d.comm) {
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(1024), 0, d.stream, (const double*)w.partials, nparts, ncomp, stage, w.scal);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(1024), 0, d.stream, (const double*)w.partials, nparts, ncomp, stage,
                     (const SolveScal*)w.scal, w.rec, (int)counters, (const int32_t*)extra);
  SOLVE_HIP(hipGetLastError());
  SOLVE_HIP(callback(d, d.comm->allreduce_sum(d.comm->user, w.rec, counters ? 6 : extra ? 5 : ncomp, (void*)d.stream)));
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, d.stream, (const double*)w.rec, stage, w.scal, (int)counters, extra);
  return hipGetLastError();
}

// the one host read of an iteration: the scalar record, behind everything enqueued so far
hipError_t read_record(const SolveDev& d, const Work& w) {
  SOLVE_HIP(hipMemcpyAsync(d.host_rec, w.scal, sizeof(SolveScal), hipMemcpyDeviceToHost, d.stream));
  return hipStreamSynchronize(d.stream);
}

// true residual of x: r = r_hat = D^-1 (b - A x), p = v = 0, scalars as at the start; this is also the restart
// (across partitions: the ghost values of x are exchanged first; first: the record carries the counters of setup; extra: finalize)
template <int NV>
hipError_t residual(const SolveDev& d, const Work& w, double* x, double scale, bool first = false, int32_t* extra = nullptr) {
  SOLVE_HIP(apply_halo<NV>(d, w, PLAIN, x, w.t, nullptr));
  if (w.node_blocks)   // a partition may own no node; the single-partition entry never gets here without one
    hipLaunchKernelGGL((k_residual<NV>), dim3((unsigned)w.node_blocks), dim3(256), 0, d.stream, d.rhs, scale, (const double*)w.t,
                       (const double*)w.dinv, w.r, w.rh, w.p, w.v, d.n_owned, w.partials);
  SOLVE_HIP(hipGetLastError());
  SOLVE_HIP(finalize(d, w, w.node_blocks, 4, STAGE_INIT, first && d.comm, d.comm ? extra : nullptr));
  return read_record(d, w);
}

// The read of a collective hook that computes no residual (solve_gmres_arnoldi across ranks): the counters of the set-up cross the
// ranks as they do behind the first residual of a solve, beside sums that are zero, so that every rank refuses or runs together.
hipError_t share_counters(const SolveDev& d, const Work& w) {
  SOLVE_HIP(finalize(d, w, 0, 4, STAGE_INIT, true));
  return read_record(d, w);
}

// D^-1 and, if wanted, the fp32 copy of D^-1 A from the current values (scal must have been cleared)
template <int NV>
hipError_t setup(const SolveDev& d, const Work& w, int precond, bool f32) {
  if (!w.node_blocks) return hipSuccess;
  hipLaunchKernelGGL((k_precond_setup<NV>), dim3((unsigned)w.node_blocks), dim3(256), 0, d.stream, d.bptr, d.bcol, d.val, d.n_owned,
                     precond, w.dinv, w.scal);
  if (f32)
    hipLaunchKernelGGL((k_scale_f32<NV>), dim3((unsigned)op_blocks(d.n_owned, F32)), dim3(256), 0, d.stream, d.bptr, d.voff, d.val,
                       (const double*)w.dinv, d.n_owned, d.val32, w.scal);
  return hipGetLastError();
}

// Across ranks: does the kernel that writes x on level l also fill the level's send buffer?  (Level 0 keeps k_halo_pack.)
inline bool packs(const SolveDev& d, int l) { return d.sized && l > 0 && d.mg->lv[l].n_send > 0; }
inline SendList send_list(const MgLevelDev& L) { return SendList{L.send_ptr, L.send_slot, L.send}; }

// y = A_l x inside the cycle.  Across ranks x is exchanged first (it is written: its ghost tail receives): level 0 as apply_halo
// does it, a level below through the sized exchange of the send buffer its last writer filled, then one launch over the owned rows.
template <int NV>
hipError_t mg_apply(const SolveDev& d, const Work& w, int l, Form form, double* x, double* y) {
  if (l == 0) return apply_halo<NV>(d, w, form, x, y, nullptr);
  if (d.sized) {
    const MgLevelDev& L = d.mg->lv[l];
    SOLVE_HIP(callback(d, d.sized->exchange_sized_begin(d.comm->user, L.send, x + L.n * NV, d.peers, L.send_off, L.ghost_off, (void*)d.stream)));
    SOLVE_HIP(callback(d, d.sized->exchange_sized_end(d.comm->user, (void*)d.stream)));
  }
  return apply<NV>(d, &w, l, form, x, y, nullptr);
}

// The sweeps of gs_sweeps on a partitioned hierarchy, one at a time behind the exchange of x.  Level 0: k_halo_pack and the exchange
// of the plan's size; with one launch per colour the nodes of colour 0 below n_int -- a prefix of its ascending list,
// MgGsDev::int0 of them -- run inside the exchange: they read no ghost, and no node of a colour reads another.  A level below: the
// sized exchange of the send buffer its last writer filled; a sweep that another follows fills it again (k_gs_pack,
// k_gs_fused_pack).  A rank that owns no node of the level launches nothing and makes every callback.
template <int NV>
hipError_t gs_sweeps_dist(const SolveDev& d, const Work& w, int l, Form form, const double* r, double* x, int sweeps) {
  const MgLevelDev& L = d.mg->lv[l];
  const MgGsLevel& C = d.gs->lv[l];
  const bool f32 = l == 0 && form == F32, fused = d.gs->fuse && L.n <= MG_GS_FUSED_NODES;
  const double* val = l ? (const double*)L.val : d.val;
  const double* dinv = l ? (const double*)L.dinv : (const double*)w.dinv;
  const int64_t* bptr = l ? L.bptr : d.bptr;
  const int32_t* bcol = l ? L.bcol : d.bcol;
  auto colour_part = [&](int64_t c0, int64_t count, bool pack) {   // the nodes C.nodes[c0 .. c0 + count), one launch
    if (count <= 0) return;
    const dim3 grid((unsigned)op_blocks(count, f32 ? F32 : SCALED)), block(256);
    if (f32)
      hipLaunchKernelGGL((k_gs_f32<NV>), grid, block, 0, d.stream, bptr, bcol, d.voff, (const float*)d.val32, r, x, C.nodes + c0, count);
    else if (pack)
      hipLaunchKernelGGL((k_gs_pack<NV>), grid, block, 0, d.stream, bptr, bcol, val, dinv, r, x, C.nodes + c0, count, send_list(L));
    else
      hipLaunchKernelGGL((l ? k_gs<NV, false> : k_gs<NV, true>), grid, block, 0, d.stream, bptr, bcol, val, dinv, r, x, C.nodes + c0, count);
  };
  for (int s = 0; s < sweeps; s++) {
    const bool pack = packs(d, l) && s + 1 < sweeps;
    int first = 0;   // the first colour that is still to run behind the exchange
    if (l == 0) {
      if (d.dist.n_send) {
        hipLaunchKernelGGL((k_halo_pack<NV>), per_thread(d.dist.n_send * NV), dim3(256), 0, d.stream, d.send_nodes, d.dist.n_send,
                           (const double*)x, w.send);
        SOLVE_HIP(hipGetLastError());
      }
      SOLVE_HIP(callback(d, d.comm->exchange_begin(d.comm->user, w.send, x + d.n_owned * NV, (void*)d.stream)));
      const bool split = !fused && L.n && C.n_colours > 0;
      if (split) colour_part(C.cptr_host[0], d.gs->int0, false);
      SOLVE_HIP(hipGetLastError());
      SOLVE_HIP(callback(d, d.comm->exchange_end(d.comm->user, (void*)d.stream)));
      if (split) {
        colour_part(C.cptr_host[0] + d.gs->int0, C.cptr_host[1] - C.cptr_host[0] - d.gs->int0, false);
        first = 1;
      }
    } else if (d.sized) {
      SOLVE_HIP(callback(d, d.sized->exchange_sized_begin(d.comm->user, L.send, x + L.n * NV, d.peers, L.send_off, L.ghost_off, (void*)d.stream)));
      SOLVE_HIP(callback(d, d.sized->exchange_sized_end(d.comm->user, (void*)d.stream)));
    }
    if (!L.n) continue;
    if (fused) {
      const dim3 one(1), block(GS_FUSED_THREADS);
      if (f32)
        hipLaunchKernelGGL((k_gs_f32_fused<NV>), one, block, 0, d.stream, bptr, bcol, d.voff, (const float*)d.val32, r, x, C.nodes, C.cptr,
                           C.n_colours, 1);
      else if (pack)
        hipLaunchKernelGGL((k_gs_fused_pack<NV>), one, block, 0, d.stream, bptr, bcol, val, dinv, r, x, C.nodes, C.cptr, C.n_colours, send_list(L));
      else
        hipLaunchKernelGGL((l ? k_gs_fused<NV, false> : k_gs_fused<NV, true>), one, block, 0, d.stream, bptr, bcol, val, dinv, r, x, C.nodes,
                           C.cptr, C.n_colours, 1);
    } else {
      for (int c = first; c < C.n_colours; c++) colour_part(C.cptr_host[c], C.cptr_host[c + 1] - C.cptr_host[c], pack);
    }
    SOLVE_HIP(hipGetLastError());
  }
  return hipSuccess;
}

// `sweeps` forward Gauss-Seidel sweeps on level l over its colour lists (d.gs): x_n += D_l^-1 (r_n - (A_l x)_n) in place.  A level
// of at most MG_GS_FUSED_NODES nodes takes one launch of one workgroup for all of them, any other one launch per colour and sweep.
// Across ranks (RDC_PRECOND_MULTIGRID_GS_LOCAL) the sweep is Gauss-Seidel inside the rank and Jacobi between the ranks: the ghost
// values a sweep reads are those of the exchange that precedes it, one per sweep as the damped-Jacobi sweep has it for its
// operator, so the callbacks of a cycle are those of mg_smooth without colour lists.
template <int NV>
hipError_t gs_sweeps(const SolveDev& d, const Work& w, int l, Form form, const double* r, double* x, int sweeps) {
  if (d.comm) return gs_sweeps_dist<NV>(d, w, l, form, r, x, sweeps);
  const MgLevelDev& L = d.mg->lv[l];
  const MgGsLevel& C = d.gs->lv[l];
  if (!L.n) return hipSuccess;
  const bool f32 = l == 0 && form == F32, fused = d.gs->fuse && L.n <= MG_GS_FUSED_NODES;
  const double* val = l ? (const double*)L.val : d.val;
  const double* dinv = l ? (const double*)L.dinv : (const double*)w.dinv;
  if (fused) {
    const dim3 one(1), block(GS_FUSED_THREADS);
    if (f32)
      hipLaunchKernelGGL((k_gs_f32_fused<NV>), one, block, 0, d.stream, L.bptr, L.bcol, d.voff, (const float*)d.val32, r, x, C.nodes, C.cptr,
                         C.n_colours, sweeps);
    else
      hipLaunchKernelGGL((l ? k_gs_fused<NV, false> : k_gs_fused<NV, true>), one, block, 0, d.stream, L.bptr, L.bcol, val, dinv, r, x, C.nodes,
                         C.cptr, C.n_colours, sweeps);
    return hipGetLastError();
  }
  for (int s = 0; s < sweeps; s++)
    for (int c = 0; c < C.n_colours; c++) {
      const int64_t c0 = C.cptr_host[c], count = C.cptr_host[c + 1] - c0;
      const dim3 grid((unsigned)op_blocks(count, f32 ? F32 : SCALED)), block(256);
      if (f32)
        hipLaunchKernelGGL((k_gs_f32<NV>), grid, block, 0, d.stream, L.bptr, L.bcol, d.voff, (const float*)d.val32, r, x, C.nodes + c0, count);
      else
        hipLaunchKernelGGL((l ? k_gs<NV, false> : k_gs<NV, true>), grid, block, 0, d.stream, L.bptr, L.bcol, val, dinv, r, x, C.nodes + c0, count);
    }
  return hipGetLastError();
}

// `sweeps` sweeps of the smoother on level l from the x at hand: damped Jacobi, x += w D_l^-1 (r - A_l x), or, with colour lists
// (d.gs), forward Gauss-Seidel, which needs neither t nor a launch of the operator
template <int NV>
hipError_t mg_smooth(const SolveDev& d, const Work& w, int l, Form form, const double* r, double* x, double* t, int sweeps = 1) {
  if (d.gs) return gs_sweeps<NV>(d, w, l, form, r, x, sweeps);
  const MgDev& g = *d.mg;
  const int64_t n = g.lv[l].n;
  for (int s = 0; s < sweeps; s++) {
    SOLVE_HIP(mg_apply<NV>(d, w, l, form, x, t));
    if (!n) continue;   // a rank may own no node of a level
    if (l == 0)
      hipLaunchKernelGGL((k_smooth<NV, true, false>), per_thread(n * NV), dim3(256), 0, d.stream, (const double*)nullptr, r, (const double*)t, g.omega, n, x);
    else if (packs(d, l))
      hipLaunchKernelGGL((k_smooth_pack<NV>), per_thread(n * NV), dim3(256), 0, d.stream, (const double*)g.lv[l].dinv, r, (const double*)t, g.omega, n, x,
                         send_list(g.lv[l]));
    else
      hipLaunchKernelGGL((k_smooth<NV, false, false>), per_thread(n * NV), dim3(256), 0, d.stream, (const double*)g.lv[l].dinv, r, (const double*)t, g.omega, n, x);
    SOLVE_HIP(hipGetLastError());
  }
  return hipSuccess;
}

// out = M in: one V(1,1) cycle from a zero start.  Enqueues only; a fixed linear operator for fixed values.  Across ranks `out`
// has a ghost tail, and with L >= 2 levels the cycle makes 2 exchanges of the plan's size and 2 (L - 2) + 7 sized ones.
template <int NV>
hipError_t mg_cycle(const SolveDev& d, const Work& w, Form form, const double* in, double* out) {
  const MgDev& g = *d.mg;
  const int last = g.n_levels - 1;
  auto R = [&](int l) { return l == 0 ? in : (const double*)g.lv[l].r; };
  auto X = [&](int l) { return l == 0 ? out : g.lv[l].x; };
  auto T = [&](int l) { return l == 0 ? g.t0 : g.lv[l].t; };
  if (w.n)
    hipLaunchKernelGGL((k_smooth<NV, true, true>), per_thread(w.n), dim3(256), 0, d.stream, (const double*)nullptr, in,
                       (const double*)nullptr, g.omega, d.n_owned, out);
  for (int l = 0; l < last; l++) {   // down: residual of the first sweep, restricted; the coarse level's first sweep rides along
    const MgLevelDev& C = g.lv[l + 1];
    SOLVE_HIP(mg_apply<NV>(d, w, l, form, X(l), T(l)));
    if (!C.n) continue;
    if (packs(d, l + 1))
      hipLaunchKernelGGL((k_restrict_pack<NV>), per_thread(C.n), dim3(256), 0, d.stream, C.mptr, C.member, R(l),
                         (const double*)T(l), (const double*)C.dinv, g.omega, C.n, C.r, C.x, send_list(C));
    else
      hipLaunchKernelGGL((k_restrict<NV>), per_thread(C.n), dim3(256), 0, d.stream, C.mptr, C.member, R(l),
                         (const double*)T(l), (const double*)C.dinv, g.omega, C.n, C.r, C.x);
  }
  SOLVE_HIP(mg_smooth<NV>(d, w, last, form, R(last), X(last), T(last), MG_COARSEST_SWEEPS - 1));
  for (int l = last - 1; l >= 0; l--) {   // up: correction, then the second sweep
    const int64_t n = g.lv[l].n;
    if (n) {
      if (packs(d, l))
        hipLaunchKernelGGL((k_prolong_pack<NV>), per_thread(n * NV), dim3(256), 0, d.stream, g.lv[l + 1].agg, (const double*)g.lv[l + 1].x, X(l), n,
                           send_list(g.lv[l]));
      else
        hipLaunchKernelGGL((k_prolong<NV>), per_thread(n * NV), dim3(256), 0, d.stream, g.lv[l + 1].agg, (const double*)g.lv[l + 1].x, X(l), n);
    }
    SOLVE_HIP(mg_smooth<NV>(d, w, l, form, R(l), X(l), T(l)));
  }
  return hipGetLastError();
}

// values and D_l^-1 of every coarse level from the current values (behind setup(): level 1 reads D^-1); counts into bad_blocks
template <int NV>
hipError_t mg_setup(const SolveDev& d, const Work& w) {
  const MgDev& g = *d.mg;
  for (int l = 1; l < g.n_levels; l++) {
    const MgLevelDev& C = g.lv[l];
    const int64_t* fbptr = l == 1 ? d.bptr : g.lv[l - 1].bptr;
    const double* fval = l == 1 ? d.val : (const double*)g.lv[l - 1].val;
    const dim3 grid = per_thread(C.blocks * NV * NV);
    if (!C.n) continue;   // across ranks: a rank may own no node of a level
    if (l == 1)
      hipLaunchKernelGGL((k_galerkin<NV, true>), grid, dim3(256), 0, d.stream, C.cptr, C.cidx, C.cnode, C.brow, C.blocks, fbptr, fval,
                         (const double*)w.dinv, C.bptr, C.val);
    else
      hipLaunchKernelGGL((k_galerkin<NV, false>), grid, dim3(256), 0, d.stream, C.cptr, C.cidx, C.cnode, C.brow, C.blocks, fbptr, fval,
                         (const double*)nullptr, C.bptr, C.val);
    hipLaunchKernelGGL((k_precond_setup<NV>), per_thread(C.n), dim3(256), 0, d.stream, C.bptr, C.bcol,
                       (const double*)C.val, C.n, (int)RDC_PRECOND_BLOCK_JACOBI, C.dinv, w.scal);
  }
  return hipGetLastError();
}

// the factor from the current values (behind setup(): the copy reads D^-1): A^ into the private layout, then one launch per colour
// in ascending order; a pivot U_ii that cannot be inverted counts into bad_blocks.  Lists with ghost columns (g.nown): the _owned
// kernels, the factor of the owned square.  A rank that owns no node launches nothing.
template <int NV>
hipError_t ilu_setup(const SolveDev& d, const Work& w) {
  const IluDev& g = *d.ilu;
  const dim3 grid((unsigned)op_blocks(d.n_owned, SCALED)), block(256);
  if (!grid.x) return hipSuccess;
  if (g.nown)
    hipLaunchKernelGGL((k_ilu_copy_owned<NV>), grid, block, 0, d.stream, d.bptr, d.bcol, g.pcol, g.nlow, g.nown, d.val, (const double*)w.dinv,
                       d.n_owned, g.val);
  else
    hipLaunchKernelGGL((k_ilu_copy<NV>), grid, block, 0, d.stream, d.bptr, d.bcol, g.pcol, g.nlow, d.val, (const double*)w.dinv, d.n_owned, g.val);
  for (int c = 0; c < g.n_colours; c++) {
    const int64_t c0 = g.cptr_host[c], count = g.cptr_host[c + 1] - c0;
    const dim3 cgrid((unsigned)op_blocks(count, SCALED));
    if (g.nown)
      hipLaunchKernelGGL((k_ilu_factor_owned<NV>), cgrid, block, 0, d.stream, d.bptr, g.pcol, g.nlow, g.nown, g.colour, g.val, g.uinv,
                         g.nodes + c0, count, w.scal);
    else
      hipLaunchKernelGGL((k_ilu_factor<NV>), cgrid, block, 0, d.stream, d.bptr, g.pcol, g.nlow, g.colour, g.val, g.uinv, g.nodes + c0, count,
                         w.scal);
  }
  if (g.want32)   // the fp32 copy the sweeps stream ("ilu_factor_bits" = 32); its overflow count travels in the record of bad_blocks
    hipLaunchKernelGGL((k_ilu_round_f32<NV>), dim3((unsigned)op_blocks(d.n_owned, F32)), block, 0, d.stream, d.bptr, g.nlow, g.nown,
                       (const double*)g.val, g.foff, d.n_owned, g.val32, w.scal);
  return hipGetLastError();
}

// out = (LU)^-1 in: forward over the colours ascending, backward descending, one launch per colour each way (colour 0 forward is the
// copy of `in`, since out is another vector).  Enqueues only; a fixed linear operator for fixed values.  Writes the owned entries
// of `out` and needs no communication: across ranks the factor is rank-local, and the ghost tail of `out` is filled by the exchange
// of the operator application that follows.  f32: the sweeps stream the fp32 copy of the factor (the same launches, 8 lanes per node).
template <int NV>
hipError_t ilu_apply(const SolveDev& d, const double* in, double* out, bool f32) {
  const IluDev& g = *d.ilu;
  const Form lanes = f32 ? F32 : SCALED;
  for (int c = 0; c < g.n_colours; c++) {
    const int64_t c0 = g.cptr_host[c], count = g.cptr_host[c + 1] - c0;
    if (f32)
      hipLaunchKernelGGL((k_ilu_fwd_f32<NV>), dim3((unsigned)op_blocks(count, lanes)), dim3(256), 0, d.stream, d.bptr, g.pcol, g.nlow, g.foff,
                         (const float*)g.val32, in, out, g.nodes + c0, count);
    else
      hipLaunchKernelGGL((k_ilu_fwd<NV>), dim3((unsigned)op_blocks(count, SCALED)), dim3(256), 0, d.stream, d.bptr, g.pcol, g.nlow,
                         (const double*)g.val, in, out, g.nodes + c0, count);
  }
  for (int c = g.n_colours - 1; c >= 0; c--) {
    const int64_t c0 = g.cptr_host[c], count = g.cptr_host[c + 1] - c0;
    if (f32 && g.nown)
      hipLaunchKernelGGL((k_ilu_bwd_f32_owned<NV>), dim3((unsigned)op_blocks(count, lanes)), dim3(256), 0, d.stream, d.bptr, g.pcol, g.nlow,
                         g.nown, g.foff, (const float*)g.val32, (const double*)g.uinv, out, g.nodes + c0, count);
    else if (f32)
      hipLaunchKernelGGL((k_ilu_bwd_f32<NV>), dim3((unsigned)op_blocks(count, lanes)), dim3(256), 0, d.stream, d.bptr, g.pcol, g.nlow, g.foff,
                         (const float*)g.val32, (const double*)g.uinv, out, g.nodes + c0, count);
    else if (g.nown)
      hipLaunchKernelGGL((k_ilu_bwd_owned<NV>), dim3((unsigned)op_blocks(count, SCALED)), dim3(256), 0, d.stream, d.bptr, g.pcol, g.nlow, g.nown,
                         (const double*)g.val, (const double*)g.uinv, out, g.nodes + c0, count);
    else
      hipLaunchKernelGGL((k_ilu_bwd<NV>), dim3((unsigned)op_blocks(count, SCALED)), dim3(256), 0, d.stream, d.bptr, g.pcol, g.nlow,
                         (const double*)g.val, (const double*)g.uinv, out, g.nodes + c0, count);
  }
  return hipGetLastError();
}

// One BiCGStab iteration.  form: what the operator applications stream (F32: the copy, which needs no D^-1 epilogue).
// right: a preconditioner M is applied from the right (the multigrid cycle, or the ILU(0) sweeps), so the operator sees M p and
// M s and x advances along them.
enum Right { RIGHT_NONE, RIGHT_MG, RIGHT_ILU };

template <int NV>
hipError_t right_apply(const SolveDev& d, const Work& w, Form form, Right right, const double* in, double* out) {
  return right == RIGHT_MG ? mg_cycle<NV>(d, w, form, in, out) : ilu_apply<NV>(d, in, out, d.ilu->bits == 32);
}

template <int NV>
hipError_t iteration(const SolveDev& d, const Work& w, double* x, Form form, Right right) {
  const bool mg = right != RIGHT_NONE;
  const dim3 vg((unsigned)w.vec_blocks), vb(256);
  const int64_t parts = op_parts(d.n_owned, d.comm ? d.dist.n_int : 0, form);
  double* px = right == RIGHT_MG ? d.mg->ph : right == RIGHT_ILU ? d.ilu->ph : w.p;   // across partitions: the ghost tails of these receive (mg_place gives M p and M s one too)
  double* sx = right == RIGHT_MG ? d.mg->sh : right == RIGHT_ILU ? d.ilu->sh : w.s;
  if (vg.x) hipLaunchKernelGGL(k_update_p, vg, vb, 0, d.stream, (const double*)w.r, w.p, (const double*)w.v, (const SolveScal*)w.scal, w.n);
  if (mg) SOLVE_HIP(right_apply<NV>(d, w, form, right, w.p, px));
  SOLVE_HIP(apply_halo<NV>(d, w, form, px, w.v, w.rh));   // v = D^-1 A [M] p, (r_hat, v)
  SOLVE_HIP(finalize(d, w, parts, 2, STAGE_ALPHA));
  if (vg.x) hipLaunchKernelGGL(k_update_s, vg, vb, 0, d.stream, (const double*)w.r, (const double*)w.v, w.s, (const SolveScal*)w.scal, w.n);
  if (mg) SOLVE_HIP(right_apply<NV>(d, w, form, right, w.s, sx));
  SOLVE_HIP(apply_halo<NV>(d, w, form, sx, w.t, w.s));    // t = D^-1 A [M] s, (t, s), (t, t)
  SOLVE_HIP(finalize(d, w, parts, 2, STAGE_OMEGA));
  if (vg.x)
    hipLaunchKernelGGL((mg ? k_update_xr<true> : k_update_xr<false>), vg, vb, 0, d.stream, x, w.r, (const double*)w.p, (const double*)w.s,
                       (const double*)w.t, (const double*)w.rh, (const SolveScal*)w.scal, w.n, w.partials, mg ? (const double*)px : nullptr,
                       mg ? (const double*)sx : nullptr);
  SOLVE_HIP(hipGetLastError());
  SOLVE_HIP(finalize(d, w, w.vec_blocks, 3, STAGE_RHO));
  return read_record(d, w);
}

// What a solve does before its first iteration, stated once for run() and for the probe of the cycle (solve_mg_apply): the scalars
// cleared, D^-1 and (mixed) the fp32 copy, with RDC_PRECOND_MULTIGRID the values and D_l^-1 of every coarse level, then `read`,
// which brings the scalar record to the host -- the first residual of a solve, the bare copy of the probe -- and what the record
// decides: the blocks that could not be inverted, and the form the operator applications stream.
struct Start {
  Form form = SCALED;
  int bad_blocks = 0;
};

template <int NV, class Read>
hipError_t prologue(const SolveDev& d, const Work& w, int precond, bool mixed, Read&& read, Start* s) {
  SOLVE_HIP(hipMemsetAsync(w.scal, 0, sizeof(SolveScal), d.stream));
  const bool mg = precond == RDC_PRECOND_MULTIGRID;   // the system is that of block Jacobi, the cycle comes on top
  const bool ilu = precond == RDC_PRECOND_ILU0 || precond == RDC_PRECOND_ILU0_LOCAL;   // ... or the ILU(0) sweeps (5: of the rank's owned square)
  SOLVE_HIP(setup<NV>(d, w, mg || ilu ? (int)RDC_PRECOND_BLOCK_JACOBI : precond, mixed));
  if (mg) SOLVE_HIP(timed(d.stream, &d.mg->setup_ms, [&] { return mg_setup<NV>(d, w); }));
  if (ilu) SOLVE_HIP(timed(d.stream, &d.ilu->setup_ms, [&] { return ilu_setup<NV>(d, w); }));
  SOLVE_HIP(read());
  s->bad_blocks = d.host_rec->bad_blocks;
  s->form = mixed && d.host_rec->f32_overflow == 0 ? F32 : SCALED;   // an entry of D^-1 A does not fit fp32: iterate on the FP64 values
  if (ilu) d.ilu->bits = d.ilu->want32 && d.host_rec->ilu_overflow == 0 ? 32 : 64;   // ... of the factor: the FP64 sweeps (this rank's own choice)
  return hipSuccess;
}

// the norms of the record into info, with the reason
void report(const SolveScal& rec, rdc_solve_info* info, int reason) {
  info->reason = reason;
  info->rhs_norm = std::sqrt(rec.bn2); info->residual_norm = std::sqrt(rec.rn2);
  info->plain_rhs_norm = std::sqrt(rec.bn2_plain); info->plain_residual_norm = std::sqrt(rec.rn2_plain);
}

// The opening of a solve, whatever its method: the prologue with the first residual, and the outcomes that need no iteration (a
// diagonal block that cannot be inverted, a residual that is not finite, b = 0, an initial guess that already passes).  *done: info
// is complete; otherwise *form is what the operator applications stream and *tol the bound on the residual norm.
template <int NV>
hipError_t open_solve(const SolveDev& d, const Work& w, const rdc_solve_params& p, double* x, rdc_solve_info* info, bool mixed, Form* form,
                      double* tol, bool* done) {
  const SolveScal& rec = *d.host_rec;
  *done = true;
  Start start;
  SOLVE_HIP(prologue<NV>(d, w, (int)p.precond, mixed, [&] { return residual<NV>(d, w, x, p.rhs_scale, true); }, &start));
  info->bad_blocks = start.bad_blocks;
  *form = start.form;
  info->matrix_bits = start.form == F32 ? 32 : 64;
  if (start.bad_blocks > 0) { report(rec, info, RDC_SOLVE_BAD_DIAGONAL); return hipSuccess; }
  if (rec.flag) { report(rec, info, RDC_SOLVE_NOT_FINITE); return hipSuccess; }
  if (rec.bn2 == 0.0) {   // b = 0: x = 0
    SOLVE_HIP(hipMemsetAsync(x, 0, (size_t)(d.comm ? d.dist.n_nodes * NV : w.n) * sizeof(double), d.stream));
    SOLVE_HIP(hipStreamSynchronize(d.stream));
    report(rec, info, RDC_SOLVE_CONVERGED);
    info->residual_norm = info->plain_residual_norm = 0.0;
    return hipSuccess;
  }
  *tol = std::max(p.rel_tol * std::sqrt(rec.bn2), p.abs_tol);
  if (std::sqrt(rec.rn2) <= *tol) { report(rec, info, RDC_SOLVE_CONVERGED); return hipSuccess; }
  *done = false;
  return hipSuccess;
}

inline Right right_of(const rdc_solve_params& p) {
  return p.precond == RDC_PRECOND_MULTIGRID ? RIGHT_MG
         : p.precond == RDC_PRECOND_ILU0 || p.precond == RDC_PRECOND_ILU0_LOCAL ? RIGHT_ILU : RIGHT_NONE;
}

template <int NV>
hipError_t run(const SolveDev& d, const rdc_solve_params& p, double* x, rdc_solve_info* info, bool mixed) {
  const Work w = carve(d.nvar, d.n_owned, d.work, d.comm ? &d.dist : nullptr);
  const SolveScal& rec = *d.host_rec;   // across partitions: the all-reduced scalars, the same bits on every rank, so every branch below is collective
  auto report = [&](int reason) { rdc::report(rec, info, reason); };
  const Right right = right_of(p);
  Form form = SCALED;
  double tol = 0.0;
  bool done = false;
  SOLVE_HIP(open_solve<NV>(d, w, p, x, info, mixed, &form, &tol, &done));
  if (done) return hipSuccess;
  int breakdowns = 0;
  for (;;) {
    if (info->iterations >= p.max_its) {
      SOLVE_HIP(residual<NV>(d, w, x, p.rhs_scale));
      report(rec.flag ? RDC_SOLVE_NOT_FINITE : (std::sqrt(rec.rn2) <= tol ? RDC_SOLVE_CONVERGED : RDC_SOLVE_MAX_ITS));
      return hipSuccess;
    }
    SOLVE_HIP(iteration<NV>(d, w, x, form, right));
    info->iterations++;
    const bool claims = !(rec.flag & 1) && std::sqrt(rec.rn2) <= tol;
    if (!claims && !rec.flag) continue;
    if (!claims && ++breakdowns > MAX_BREAKDOWNS) {
      SOLVE_HIP(residual<NV>(d, w, x, p.rhs_scale));
      report(rec.flag ? RDC_SOLVE_NOT_FINITE : RDC_SOLVE_BREAKDOWN);
      return hipSuccess;
    }
    // the recurrence says "converged", or it broke down: the TRUE residual of x decides, and is the restart
    SOLVE_HIP(residual<NV>(d, w, x, p.rhs_scale));
    if (rec.flag) { report(RDC_SOLVE_NOT_FINITE); return hipSuccess; }
    if (std::sqrt(rec.rn2) <= tol) { report(RDC_SOLVE_CONVERGED); return hipSuccess; }
    info->restarts++;
  }
}

// ---- restarted GMRES(m), host side ----

// the one host read of an Arnoldi step: the record, behind everything enqueued so far
hipError_t gmres_read(const SolveDev& d, const GmresState& G) {
  SOLVE_HIP(hipMemcpyAsync(d.gmres_rec, G.rec, sizeof(GmresRec), hipMemcpyDeviceToHost, d.stream));
  return hipStreamSynchronize(d.stream);
}

// v_0 = src / beta, g = beta e_0: the start of a cycle (beta2: device address of beta^2)
hipError_t gmres_start(const SolveDev& d, const GmresState& G, const double* src, const double* beta2) {
  hipLaunchKernelGGL(k_gmres_start, dim3((unsigned)std::max<int64_t>(G.vec_blocks, 1)), dim3(256), 0, d.stream, src, beta2, G.V, G.n, G);
  return hipGetLastError();
}

// What a step does with the partials of the kernel before it (GMRES_STAGE_*).  With a communicator the sums cross the ranks on their
// way: k_gmres_reduce, the wide all-reduce of `ncomp` doubles in place in G.red, k_gmres_advance.
hipError_t gmres_finalize(const SolveDev& d, const GmresState& G, int ncomp, int stage, int j) {
  if (!d.comm) {
    hipLaunchKernelGGL(k_gmres_finalize, dim3(1), dim3(1024), 0, d.stream, (const double*)G.partials, G.vec_blocks, ncomp, stage, j, G);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_gmres_reduce, dim3(1), dim3(1024), 0, d.stream, (const double*)G.partials, G.vec_blocks, ncomp, stage, G);
  SOLVE_HIP(hipGetLastError());
  SOLVE_HIP(callback(d, d.wide->allreduce_sum_wide(d.comm->user, G.red, ncomp, (void*)d.stream)));
  hipLaunchKernelGGL(k_gmres_advance, dim3(1), dim3(64), 0, d.stream, stage, j, G);
  return hipGetLastError();
}

// Arnoldi step j: w = D^-1 A (M v_j) into slot j + 1, one or two classical Gram-Schmidt passes against v_0 .. v_j, the norm, the
// Givens step, the scaling, and the record on the host.  Vector passes with one Gram-Schmidt pass, beside the operator and M:
// (j + 2) reads for the inner products, (j + 2) reads and 1 write for the update, 1 read and 1 write for the scaling: 2 j + 7.
// Across ranks the operator's exchange receives into the ghost tail of v_j itself (or of M v_j), the sums run over the owned
// entries, and a step makes one wide all-reduce per Gram-Schmidt pass (j + 2 doubles) and one for the norm (1 double).  A rank that
// owns no node launches no vector kernel and adds zeros.
template <int NV>
hipError_t gmres_step(const SolveDev& d, const Work& w, const GmresState& G, Form form, Right right, int j) {
  double* vj = G.V + (int64_t)j * G.stride;
  double* wn = G.V + (int64_t)(j + 1) * G.stride;
  double* in = vj;
  if (right != RIGHT_NONE) {
    in = right == RIGHT_MG ? d.mg->ph : d.ilu->ph;
    SOLVE_HIP(right_apply<NV>(d, w, form, right, vj, in));
  }
  SOLVE_HIP(apply_halo<NV>(d, w, form, in, wn, nullptr));
  const dim3 vg((unsigned)G.vec_blocks), vb(256);
  for (int pass = 0; pass < (d.gmres_refine ? 2 : 1); pass++) {
    if (vg.x) hipLaunchKernelGGL(k_gmres_dots, vg, vb, 0, d.stream, (const double*)G.V, G.stride, j + 1, (const double*)wn, G.n, G.partials, G.vec_blocks);
    SOLVE_HIP(gmres_finalize(d, G, j + 2, pass ? (int)GMRES_STAGE_DOTS2 : (int)GMRES_STAGE_DOTS, j));
    if (vg.x) hipLaunchKernelGGL(k_gmres_orth, vg, vb, 0, d.stream, (const double*)G.V, G.stride, j + 1, wn, G.n, (const double*)G.hpass, G.partials,
                                 (const GmresRec*)G.rec);
  }
  SOLVE_HIP(gmres_finalize(d, G, 1, (int)GMRES_STAGE_NORM, j));
  if (vg.x) hipLaunchKernelGGL(k_gmres_scale, vg, vb, 0, d.stream, wn, G.n, (const double*)(G.scal + 1), (const GmresRec*)G.rec);
  SOLVE_HIP(hipGetLastError());
  return gmres_read(d, G);
}

// The Arnoldi steps of one cycle from v_0: until stop(steps taken) says so, a step is flagged, or `max_steps` are taken.  *taken:
// the columns that may be used (a step flagged NOT_FINITE or SINGULAR is not among them); *run: the operator applications.
template <int NV, class Stop>
hipError_t gmres_arnoldi(const SolveDev& d, const Work& w, const GmresState& G, Form form, Right right, int max_steps, Stop&& stop,
                         int* taken, int* run) {
  const GmresRec& rec = *d.gmres_rec;
  *taken = *run = 0;
  while (*taken < max_steps) {
    SOLVE_HIP(gmres_step<NV>(d, w, G, form, right, *taken));
    ++*run;
    if (rec.flag & (GMRES_NOT_FINITE | GMRES_SINGULAR)) break;
    ++*taken;
    if ((rec.flag & GMRES_HAPPY) || stop(*taken)) break;
  }
  return hipSuccess;
}

// x += M (V y) for the leading k columns: the back substitution, the sum (fused into the update of x without a right
// preconditioner), one application of M.  Enqueues only; the record (overflow, a y that is not finite) travels with the next read.
template <int NV>
hipError_t gmres_update(const SolveDev& d, const Work& w, const GmresState& G, Form form, Right right, int k, double* x) {
  const dim3 vg((unsigned)G.vec_blocks), vb(256);
  hipLaunchKernelGGL(k_gmres_solve_y, dim3(1), dim3(64), 0, d.stream, k, G);
  if (right == RIGHT_NONE) {
    if (vg.x) hipLaunchKernelGGL((k_gmres_combine<true>), vg, vb, 0, d.stream, (const double*)G.V, G.stride, k, (const double*)G.y, x, G.n, G.rec);
  } else {
    double* z = right == RIGHT_MG ? d.mg->ph : d.ilu->ph;
    if (vg.x) hipLaunchKernelGGL((k_gmres_combine<false>), vg, vb, 0, d.stream, (const double*)G.V, G.stride, k, (const double*)G.y, w.s, G.n, G.rec);
    SOLVE_HIP(right_apply<NV>(d, w, form, right, w.s, z));
    if (vg.x) hipLaunchKernelGGL((k_gmres_combine<true>), vg, vb, 0, d.stream, (const double*)z, (int64_t)0, 1, (const double*)(G.scal + 2), x, G.n, G.rec);
  }
  SOLVE_HIP(hipGetLastError());
  return hipMemcpyAsync(d.gmres_rec, G.rec, sizeof(GmresRec), hipMemcpyDeviceToHost, d.stream);
}

// Right-preconditioned GMRES(m) on the system of run(): every cycle starts from the true FP64 residual, which also decides.
// Across ranks (rdc_solve_dist_gmres) both records hold all-reduced values, the same bits on every rank, so every branch below is
// collective; the one rank-local value, the overflow count of the update of x, becomes global in the all-reduce of the true
// residual behind it and is read once more after that.
template <int NV>
hipError_t run_gmres(const SolveDev& d, const rdc_solve_params& p, double* x, rdc_solve_info* info, bool mixed) {
  const Work w = carve(d.nvar, d.n_owned, d.work, d.comm ? &d.dist : nullptr);
  GmresState& G = *d.gmres;
  const SolveScal& rec = *d.host_rec;
  const GmresRec& grec = *d.gmres_rec;
  const Right right = right_of(p);
  Form form = SCALED;
  double tol = 0.0;
  bool done = false;
  G.cycles = 0;
  SOLVE_HIP(open_solve<NV>(d, w, p, x, info, mixed, &form, &tol, &done));
  if (done) return hipSuccess;
  for (;;) {
    G.cycles++;
    SOLVE_HIP(gmres_start(d, G, w.r, &w.scal->rn2));
    int k = 0, steps = 0;
    const int left = p.max_its - info->iterations;   // >= 1: a cycle always takes a step
    SOLVE_HIP(gmres_arnoldi<NV>(d, w, G, form, right, std::min(G.restart, left), [&](int) { return grec.est <= tol; }, &k, &steps));
    info->iterations += steps;
    const int step_flag = grec.flag;
    if (k > 0) SOLVE_HIP(gmres_update<NV>(d, w, G, form, right, k, x));
    SOLVE_HIP(residual<NV>(d, w, x, p.rhs_scale, false, k > 0 ? &G.rec->overflow : nullptr));   // the true residual of x decides, and is the next cycle's start
    if (d.comm && k > 0) SOLVE_HIP(gmres_read(d, G));
    if (rec.flag || (step_flag & GMRES_NOT_FINITE) || (k > 0 && (grec.overflow || (grec.flag & GMRES_Y_NOT_FINITE)))) {
      report(rec, info, RDC_SOLVE_NOT_FINITE);
      return hipSuccess;
    }
    if (std::sqrt(rec.rn2) <= tol) { report(rec, info, RDC_SOLVE_CONVERGED); return hipSuccess; }
    if (step_flag & GMRES_SINGULAR) { report(rec, info, RDC_SOLVE_BREAKDOWN); return hipSuccess; }
    if (info->iterations >= p.max_its) { report(rec, info, RDC_SOLVE_MAX_ITS); return hipSuccess; }
    info->restarts++;
  }
}

}  // namespace

size_t solve_work_bytes(int nvar, int64_t n_owned, const DistDims* dist) { return carve(nvar, n_owned, nullptr, dist).bytes; }

hipError_t solve_matvec(const SolveDev& d, const double* x, double* y) {
  return by_nvar(d.nvar, [&](auto nv) { return apply<decltype(nv)::value>(d, nullptr, 0, PLAIN, x, y, nullptr); });
}

hipError_t solve_matvec_f32(const SolveDev& d, const double* x, double* y) {
  return by_nvar(d.nvar, [&](auto nv) { return apply<decltype(nv)::value>(d, nullptr, 0, F32, x, y, nullptr); });
}

hipError_t solve_scale_f32(const SolveDev& d, int precond, int* bad_blocks, int* overflow) {
  const Work w = carve(d.nvar, d.n_owned, d.work);
  SOLVE_HIP(hipMemsetAsync(w.scal, 0, sizeof(SolveScal), d.stream));
  SOLVE_HIP(by_nvar(d.nvar, [&](auto nv) { return setup<decltype(nv)::value>(d, w, precond, true); }));
  SOLVE_HIP(read_record(d, w));
  *bad_blocks = d.host_rec->bad_blocks;
  *overflow = d.host_rec->f32_overflow;
  return hipSuccess;
}

hipError_t solve_mg_apply(const SolveDev& d, bool mixed, const double* in, double* out, int* bad_blocks, int* matrix_bits) {
  return by_nvar(d.nvar, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    const Work w = carve(d.nvar, d.n_owned, d.work);
    Start start;
    SOLVE_HIP(prologue<NV>(d, w, (int)RDC_PRECOND_MULTIGRID, mixed, [&] { return read_record(d, w); }, &start));
    *bad_blocks = start.bad_blocks;
    *matrix_bits = start.form == F32 ? 32 : 64;
    if (start.bad_blocks > 0) return hipSuccess;   // as the solve: nothing is applied, `out` stays what it was
    SOLVE_HIP(mg_cycle<NV>(d, w, start.form, in, out));
    return hipStreamSynchronize(d.stream);
  });
}

hipError_t solve_ilu_apply(const SolveDev& d, const double* in, double* out, int* bad_blocks) {
  return by_nvar(d.nvar, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    const Work w = carve(d.nvar, d.n_owned, d.work);
    Start start;
    SOLVE_HIP(prologue<NV>(d, w, (int)RDC_PRECOND_ILU0, false, [&] { return read_record(d, w); }, &start));
    *bad_blocks = start.bad_blocks;
    if (start.bad_blocks > 0) return hipSuccess;   // as the solve: nothing is applied, `out` stays what it was
    SOLVE_HIP(ilu_apply<NV>(d, in, out, d.ilu->bits == 32));
    return hipStreamSynchronize(d.stream);
  });
}

const double* solve_dinv(const SolveDev& d) { return carve(d.nvar, d.n_owned, d.work).dinv; }

hipError_t solve_halo_pack(int nvar, const int32_t* send_nodes, int64_t n_send, const double* x, double* send, hipStream_t stream) {
  if (nvar != 3 && nvar != 5) return hipErrorInvalidValue;
  if (n_send <= 0) return hipSuccess;
  if (nvar == 3) hipLaunchKernelGGL((k_halo_pack<3>), per_thread(n_send * 3), dim3(256), 0, stream, send_nodes, n_send, x, send);
  else hipLaunchKernelGGL((k_halo_pack<5>), per_thread(n_send * 5), dim3(256), 0, stream, send_nodes, n_send, x, send);
  return hipGetLastError();
}

hipError_t solve_run(const SolveDev& d, const rdc_solve_params& p, double* x, rdc_solve_info* info, bool mixed) {
  *info = rdc_solve_info();
  info->matrix_bits = 64;
  return timed(d.stream, &info->device_ms, [&] {
    return by_nvar(d.nvar, [&](auto nv) {
      constexpr int NV = decltype(nv)::value;
      return d.gmres ? run_gmres<NV>(d, p, x, info, mixed) : run<NV>(d, p, x, info, mixed);
    });
  });
}

hipError_t solve_gmres_arnoldi(const SolveDev& d, int precond, bool mixed, const double* v0, int steps, double* V, double* H,
                               int* steps_done, int* bad_blocks, int* matrix_bits) {
  return by_nvar(d.nvar, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    const Work w = carve(d.nvar, d.n_owned, d.work, d.comm ? &d.dist : nullptr);
    const GmresState& G = *d.gmres;
    rdc_solve_params p = rdc_solve_params();
    p.precond = precond;
    const Right right = right_of(p);
    Start start;
    SOLVE_HIP(prologue<NV>(d, w, precond, mixed, [&] { return d.comm ? share_counters(d, w) : read_record(d, w); }, &start));
    *bad_blocks = start.bad_blocks;
    *matrix_bits = start.form == F32 ? 32 : 64;
    *steps_done = 0;
    if (start.bad_blocks > 0) return hipSuccess;   // as the solve: nothing is run
    const size_t hbytes = (size_t)(G.restart + 1) * G.restart * sizeof(double);
    SOLVE_HIP(hipMemsetAsync(G.H, 0, hbytes, d.stream));
    if (G.vec_blocks)
      hipLaunchKernelGGL(k_gmres_dots, dim3((unsigned)G.vec_blocks), dim3(256), 0, d.stream, (const double*)G.V, G.stride, 0, v0, G.n, G.partials,
                         G.vec_blocks);
    SOLVE_HIP(gmres_finalize(d, G, 1, (int)GMRES_STAGE_START, 0));
    SOLVE_HIP(gmres_start(d, G, v0, G.scal));
    SOLVE_HIP(gmres_read(d, G));
    int run = 0;
    if (!(d.gmres_rec->flag & GMRES_NOT_FINITE))
      SOLVE_HIP(gmres_arnoldi<NV>(d, w, G, start.form, right, steps, [](int) { return false; }, steps_done, &run));
    if (G.stride == std::max<int64_t>(G.n, 1)) {
      SOLVE_HIP(hipMemcpyAsync(V, G.V, (size_t)(*steps_done + 1) * G.stride * sizeof(double), hipMemcpyDeviceToDevice, d.stream));
    } else if (G.n) {   // ghosted slots: the owned rows of every vector, one behind the other
      SOLVE_HIP(hipMemcpy2DAsync(V, (size_t)G.n * sizeof(double), G.V, (size_t)G.stride * sizeof(double), (size_t)G.n * sizeof(double),
                                 (size_t)(*steps_done + 1), hipMemcpyDeviceToDevice, d.stream));
    }
    SOLVE_HIP(hipMemcpyAsync(H, G.H, hbytes, hipMemcpyDeviceToHost, d.stream));
    return hipStreamSynchronize(d.stream);
  });
}

}  // namespace rdc
