// rdc_cl_phases.h — the device-only phases that k_hex8_cl, k_hex8_clp, k_hex8_cl_rows (rdc_hex8_cl_kernel.h) and k_solid_cl
// (rdc_solid_cl.hip) share.  The format of the lists they decode is cll:: (rdc_prep.h), which the host builder and the CPU replay
// compile too.  No helper holds a workgroup barrier but lds_barrier itself: the kernels spell their barrier sequences out.
#ifndef RDC_CL_PHASES_H
#define RDC_CL_PHASES_H
#include "rdc_internal.h"

namespace rdc {

// block (a, b) of the model is structurally non-zero (any of the A / B / D coefficient masks)
template <class M>
constexpr bool hex8_cl_block(int a, int b) {
  bool nz = M::hasA(a, b) || M::hasD(a, b);
  for (int g = 0; g < M::NG; g++) nz = nz || M::hasB(a, b, g);
  return nz;
}

namespace cll {
typedef double v2d_t __attribute__((ext_vector_type(2)));

// Thread id by ROLE (consumer waves first) in a workgroup of NW waves.  The hardware places wave i of every workgroup on SIMD i, so
// with fixed roles the producers of the workgroups of a CU (the longer instruction stream) would share a SIMD: roles rotate
// over the waves from workgroup to workgroup.  `extra`: what the persistent form adds to tell the two workgroups of a CU apart
template <int NW>
__device__ __forceinline__ int role_tid(const unsigned extra = 0) {
  return (int)(((threadIdx.x >> 6) + (((blockIdx.x >> 3) + extra) % NW)) % NW) * 64 + (int)(threadIdx.x & 63);
}

// workgroup barrier that orders LDS accesses only (no wait for the global stores in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// image + rhs entries at `img` zeroed by the NT threads x = 0 .. NT - 1
template <int NT>
__device__ __forceinline__ void zero_image(double* img, const int x0, const int row_doubles, const int rhs_doubles) {
  v2d_t* z = reinterpret_cast<v2d_t*>(img);
  const v2d_t zero = {0.0, 0.0};
  for (int x = x0; x < zero_doubles(row_doubles, rhs_doubles) / 2; x += NT) z[x] = zero;
}

// Copy-out by NT threads, a half-wave per node: its NV rows are NV^2 * len consecutive doubles of the CSR array, written with 16-byte
// non-temporal stores (the node's image segment has the 16-byte phase of its CSR segment: odd head and tail doubles apart) or,
// `narrow` (timing comparison), with 8-byte ones; its rhs entries follow.  ntab: the cluster's table
template <int NV, int NT>
__device__ __forceinline__ void copy_out(const HostPrepCl::Node* __restrict__ ntab, const int nown, const int tid, const double* img,
                                         const double* lrhs, double* __restrict__ val, double* __restrict__ rhs, const bool narrow) {
  for (int a = tid >> 5; a < nown; a += NT / 32) {
    const HostPrepCl::Node nd = ntab[a];
    const int nn = NV * NV * (int)nd.len, l32 = tid & 31;
    double* dst = val + (int64_t)(NV * NV) * nd.bptr;
    const double* src = img + nd.off;
    const int sh = seg_phase(nd.off), npair = (nn - sh) >> 1;
    const v2d_t* s2 = reinterpret_cast<const v2d_t*>(src + sh);
    v2d_t* d2 = reinterpret_cast<v2d_t*>(dst + sh);
    if (narrow) {
      for (int x = l32; x < nn; x += 32) __builtin_nontemporal_store(src[x], dst + x);
    } else {
      for (int x = l32; x < npair; x += 32) __builtin_nontemporal_store(s2[x], d2 + x);
      if (sh && l32 == 0) __builtin_nontemporal_store(src[0], dst);
      if (((nn - sh) & 1) && l32 == 1) __builtin_nontemporal_store(src[nn - 1], dst + nn - 1);
    }
    if (l32 < NV) rhs[(int64_t)NV * nd.node + l32] = lrhs[NV * a + l32];
  }
}

// producer of a reaction-diffusion kernel: the lane's element e -> its per-element inputs; coordinates, unknowns, aux values of its nodes
template <class M>
__device__ __forceinline__ const double* elem_data(const double* elem, const uint32_t e) { return M::NELEM > 0 ? elem + (int64_t)e * M::NELEM : nullptr; }
template <class M>
__device__ __forceinline__ void load_element(const MeshDev& m, const uint32_t e, const double* __restrict__ u, const double* __restrict__ aux,
                                             double (&X)[8][3], double (&U)[8][M::NV], double (&AX)[8][M::NAUX > 0 ? M::NAUX : 1]) {
#pragma unroll
  for (int n = 0; n < 8; n++) {
    const int64_t I = m.conn[(int64_t)e * 8 + n];
#pragma unroll
    for (int c = 0; c < 3; c++) X[n][c] = m.xyz[3 * I + c];
#pragma unroll
    for (int v = 0; v < M::NV; v++) U[n][v] = u[M::NV * I + v];
#pragma unroll
    for (int v = 0; v < (M::NAUX > 0 ? M::NAUX : 1); v++)
      AX[n][v] = (M::NAUX > 0 && (M::AUX_LOCAL_NODE < 0 || n == M::AUX_LOCAL_NODE)) ? aux[(int64_t)M::NAUX * I + (M::NAUX > 0 ? v : 0)] : 0.0;
  }
}

// consumer: the lane's pair (idle lanes: valid = false, everything else 0) ...
struct Pair { bool valid; int le, li, na; };   // local element, local row node, owned-node index
__device__ __forceinline__ Pair pair_decode(const uint32_t w) {
  Pair p = {w != IDLE, 0, 0, 0};
  if (p.valid) { p.le = pair_elem(w); p.li = pair_row(w); p.na = pair_node(w); }
  return p;
}
// ... and where it adds: its slot words, its node's image segment (offset; blocks in the row).  pslot / ntab: the cluster's lists as
// 32-bit words, in memory or as k_hex8_clp stages them in LDS; x: the pair's position
struct Aim { uint32_t sl0, sl1; int off, len; };
__device__ __forceinline__ Aim pair_aim(const uint32_t* pslot, const uint32_t* ntab, const int x, const int na) {
  const uint32_t w1 = ntab[NODE_WORDS * na + 1];
  return {pslot[pslot_words(8) * x], pslot[pslot_words(8) * x + 1], node_word_off(w1), node_word_len(w1)};
}

// the pair's NV rows (acc[a][b][j]: entry (a, b) of the block of local column node j) and rhs entries added into the image;
// structurally zero blocks stay the zeros of the image
template <class M>
__device__ __forceinline__ void add_rows(double* img, double* lrhs, const Aim& t, const int na, const double (&acc)[M::NV][M::NV][8],
                                         const double (&fe)[M::NV]) {
  constexpr int NV = M::NV;
  const int lenv = NV * t.len;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    double* p = img + t.off + NV * pslot_get(t.sl0, t.sl1, j);
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++)
        if (hex8_cl_block<M>(a, b)) __hip_atomic_fetch_add(p + a * lenv + b, acc[a][b][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
#pragma unroll
  for (int a = 0; a < NV; a++) __hip_atomic_fetch_add(lrhs + NV * na + a, fe[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace cll
}  // namespace rdc
#endif
