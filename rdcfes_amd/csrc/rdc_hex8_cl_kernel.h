// rdc_hex8_cl_kernel.h — the kernel of rdc_hex8_cl.h (HIP only; included by rdc_launch.h).
#ifndef RDC_HEX8_CL_KERNEL_H
#define RDC_HEX8_CL_KERNEL_H
#include "rdc_hex8_cl.h"
#include "rdc_cl_phases.h"

#include <type_traits>

namespace rdc {

template <class M, int EXP_MODE, int CW, int PW, int PPR>
__global__ void __launch_bounds__((CW + PW) * 64, 2)
k_hex8_cl(const MeshDev m, const typename M::K k, const HostPrepCl::Desc* __restrict__ desc, const HostPrepCl::Node* __restrict__ ntab,
          const uint32_t* __restrict__ eid, const uint32_t* __restrict__ pair, const uint32_t* __restrict__ pslot,
          const double* __restrict__ u, const double* __restrict__ aux, const double* __restrict__ elem,
          double* __restrict__ val, double* __restrict__ rhs, const int diag /* "ablate" option: 64 = copy-out with 8-byte stores (timing comparison) */) {
  constexpr int NV = M::NV, NA = (M::NAUX > 0 ? M::NAUX : 1), NT = (CW + PW) * 64;
  constexpr cll::Strides S = cll::strides(CW, PW);
  constexpr int MAXP = (int)S.pair, MAXE = (int)S.elem;
  using R = Hex8Rec<M>;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int w = blockIdx.x;
  const int tid = cll::role_tid<CW + PW>();
  const HostPrepCl::Desc d = desc[w];
  const int nimg = (int)d.row_doubles, nown = (int)d.nown;
  // the image of the CSR rows of all owned nodes, and behind it their rhs entries (cll::rhs_offset, formed where it is used: held from
  // here on it is one more scalar to spill in the fast-exp instantiations), overlay the point buffers once the points are consumed
  double* const img = lds;
  // Two code paths with the SAME sequence of workgroup barriers (the branch is uniform per wave): the register allocator
  // never holds the consumers' accumulators and the producers' element at once.
  if (tid >= MAXP) {
    const int pl = tid - MAXP;
    const uint32_t e = eid[(size_t)w * S.elem + pl];
    const bool plive = e != cll::IDLE;
    double X[8][3], U[8][NV], AX[8][NA];
    if (plive) cll::load_element<M>(m, e, u, aux, X, U, AX);
    const double* ED = cll::elem_data<M>(elem, e);
    // PPR points per round and barrier: buffer (round & 1) holds the records [point in round][element]
    if (plive) {
#pragma unroll
      for (int x = 0; x < PPR; x++) hex8_cl_produce<M>(k, X, U, AX, ED, x, lds + (x * MAXE + pl) * R::STRIDE);
    }
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < 8; q += PPR) {   // one round ahead of the consumers
      if (plive && q + PPR < 8) {
#pragma unroll
        for (int x = 0; x < PPR; x++)
          hex8_cl_produce<M>(k, X, U, AX, ED, q + PPR + x, lds + (((((q / PPR) + 1) & 1) * PPR + x) * MAXE + pl) * R::STRIDE);
      }
      __syncthreads();
    }
    cll::zero_image<NT>(lds, tid, nimg, NV * nown);
    cll::lds_barrier();
    cll::lds_barrier();             // consumers: atomics
    cll::copy_out<NV, NT>(ntab + (size_t)w * S.node, nown, tid, img, img + cll::rhs_offset(nimg), val, rhs, diag & 64);
    return;
  }
  // ---- consumer: one (owned node, element) pair per lane -----------------------------------------------------------------
  double acc[NV][NV][8], fe[NV];
  rd_row_zero<M, 8>(acc, fe);
  const cll::Pair pr = cll::pair_decode(pair[(size_t)w * S.pair + tid]);
  __syncthreads();                  // producers: the first round of points
#pragma unroll 1
  for (int q = 0; q < 8; q += PPR) {
    if (pr.valid) {
#pragma unroll
      for (int x = 0; x < PPR; x++)
        hex8_cl_consume<M, EXP_MODE>(k, lds + ((((q / PPR) & 1) * PPR + x) * MAXE + pr.le) * R::STRIDE, q + x, pr.li, acc, fe);
    }
    __syncthreads();
  }
  cll::zero_image<NT>(lds, tid, nimg, NV * nown);
  cll::Aim aim = {0, 0, 0, 0};
  if (pr.valid) aim = cll::pair_aim(pslot + (size_t)w * S.pslot, reinterpret_cast<const uint32_t*>(ntab + (size_t)w * S.node), tid, pr.na);
  double* const lrhs = img + cll::rhs_offset(nimg);
  cll::lds_barrier();
  if (pr.valid) cll::add_rows<M>(img, lrhs, aim, pr.na, acc, fe);
  cll::lds_barrier();
  cll::copy_out<NV, NT>(ntab + (size_t)w * S.node, nown, tid, img, lrhs, val, rhs, diag & 64);
}

// ---- persistent form ("hex_kernel" = 2) ------------------------------------------------------------------------------------------
// In k_hex8_cl the zero / atomics / copy-out epilogue of a cluster and the drain of its stores are serial inside the
// workgroup and only overlap with the other workgroup of the CU: for the cheap integrands they cost more than the
// arithmetic.  Measured on H(126) this form ties with k_hex8_cl (HCC 2.9 vs 2.8 ms: the consumer waves' own instruction
// stream -- copy, accumulate, atomics -- is the critical path either way), so it is not the default.  A workgroup walks over the clusters blockIdx.x, blockIdx.x + gridDim.x, ..., the image has its own LDS
// region, and the memory instructions are split by role so that no wave ever waits for a store:
//   * the PRODUCER wave issues every global LOAD: its elements (fetched for the next cluster when it has no point left to
//     produce) and the work lists of the next cluster, which it passes on through LDS (three list buffers: previous,
//     current, next cluster);
//   * the CONSUMER waves issue every global STORE: while they accumulate cluster n they copy the image of cluster n - 1
//     out (one node per wave and quadrature point, zeroing what they have read), then add their rows of cluster n into
//     the image and go straight on.  vmcnt counts loads and stores in order on gfx9, so a wave that loaded after it
//     stored would wait for its stores to land; these waves never load.
// Nine workgroup barriers per cluster (LDS ordering only), none for an epilogue.
template <int CW>
struct Hex8ClLists {   // one list buffer in LDS (32-bit words)
  static constexpr int PAIR = 0, SLOT = cll::max_pairs(CW), NTAB = SLOT + cll::pslot_words(8) * cll::max_pairs(CW),
                       NOWN = NTAB + cll::NODE_WORDS * cll::max_nodes(CW), WORDS = (NOWN + 4 + 3) & ~3;
};

template <class M, int EXP_MODE, int CW, int PW>
__global__ void __launch_bounds__((CW + PW) * 64, 2)
k_hex8_clp(const MeshDev m, const typename M::K k, const HostPrepCl::Desc* __restrict__ desc, const HostPrepCl::Node* __restrict__ ntab,
           const uint32_t* __restrict__ eid, const uint32_t* __restrict__ pair, const uint32_t* __restrict__ pslot,
           const double* __restrict__ u, const double* __restrict__ aux, const double* __restrict__ elem,
           double* __restrict__ val, double* __restrict__ rhs, const int n_wg, const int img_doubles,
           const int diag /* timing diagnostics ("ablate" option), bit mask: 1 = consumers idle, 2 = producers idle, 8 = no atomics, 16 = no copy-out */) {
  constexpr int NV = M::NV, NA = (M::NAUX > 0 ? M::NAUX : 1);
  constexpr cll::Strides S = cll::strides(CW, PW);
  constexpr int MAXP = (int)S.pair, MAXE = (int)S.elem, MAXN = (int)S.node;
  static_assert(PW == 1, "one producer wave");
  using R = Hex8Rec<M>;
  using L = Hex8ClLists<CW>;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int PBUF = cll::even(2 * MAXE * R::STRIDE);
  double* const img = lds + PBUF;
  double* const lrhs = img + img_doubles;          // img_doubles = cll::rhs_offset(largest image): even
  uint32_t* const lists = reinterpret_cast<uint32_t*>(lrhs + cll::even(NV * MAXN));
  int w = blockIdx.x;
  const int G = gridDim.x;
  // workgroups b and b + gridDim.x / 2 share a CU when two are resident per CU: their producers sit on different SIMDs
  const int tid = cll::role_tid<CW + PW>(2 * blockIdx.x >= gridDim.x ? 1 : 0);
  // node a of the image of the cluster whose lists are in buffer b: copied out by one wave as runs of consecutive doubles, zeroed.
  // Not cll::copy_out: a whole wave per node, the table in LDS, and the image is zeroed as it is read (8-byte accesses)
  auto copy_node = [&](int b, int a, bool zero) {
    const uint32_t* lb = lists + b * L::WORDS;
    const int ln = tid & 63;
    if (a >= (int)lb[L::NOWN] || (diag & 16)) return;
    const uint32_t* nd = lb + L::NTAB + cll::NODE_WORDS * a;
    const uint32_t bptr = nd[0], node = nd[2];
    const int nn = NV * NV * cll::node_word_len(nd[1]), off = cll::node_word_off(nd[1]);
    double* dst = val + (int64_t)(NV * NV) * bptr;
    double v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = (ln + 64 * i < nn) ? img[off + ln + 64 * i] : 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (ln + 64 * i < nn) {
        __builtin_nontemporal_store(v[i], dst + ln + 64 * i);
        if (zero) img[off + ln + 64 * i] = 0.0;
      }
    for (int x = ln + 256; x < nn; x += 64) {   // rows longer than 28 blocks (unstructured meshes)
      __builtin_nontemporal_store(img[off + x], dst + x);
      if (zero) img[off + x] = 0.0;
    }
    if (ln < NV) {
      rhs[(int64_t)NV * node + ln] = lrhs[NV * a + ln];
      if (zero) lrhs[NV * a + ln] = 0.0;
    }
  };
  // slice s of that image = nodes s, s + 8, s + 16: one per consumer wave (a single wave -- the producer -- copying all of
  // it was measured: 3.7 instead of 2.9 ms, one wave does not keep enough stores in flight)
  auto copy_slice = [&](int b, int s, bool zero) { copy_node(b, s + 8 * (tid >> 6), zero); };
  if (tid >= MAXP) {
    // ================= producer: every global load of the workgroup ===================================================================
    const int pl = tid - MAXP;
    bool plive = false;
    double X[8][3], U[8][NV], AX[8][NA];
    const double* ED = nullptr;
    auto load_element = [&](int ww) {
      const uint32_t e = eid[(size_t)ww * S.elem + pl];
      plive = e != cll::IDLE;
      if (!plive) return;
      cll::load_element<M>(m, e, u, aux, X, U, AX);
      ED = cll::elem_data<M>(elem, e);
    };
    // work lists of cluster ww -> list buffer b
    auto stage_lists = [&](int ww, int b) {
      uint32_t* lb = lists + b * L::WORDS;
      const uint32_t* gp = pair + (size_t)ww * S.pair;
      const uint32_t* gs = pslot + (size_t)ww * S.pslot;
      const uint32_t* gn = reinterpret_cast<const uint32_t*>(ntab + (size_t)ww * S.node);
#pragma unroll
      for (int i = 0; i < CW; i++) lb[L::PAIR + pl + 64 * i] = gp[pl + 64 * i];
#pragma unroll
      for (int i = 0; i < 2 * CW; i++) lb[L::SLOT + pl + 64 * i] = gs[pl + 64 * i];
      for (int x = pl; x < cll::NODE_WORDS * MAXN; x += 64) lb[L::NTAB + x] = gn[x];
      if (pl == 0) lb[L::NOWN] = desc[ww].nown;
    };
    cll::zero_image<64>(img, pl, img_doubles, NV * MAXN);
    stage_lists(w, 0);
    load_element(w);
    int cb = 0;                             // list buffer of the current cluster
    for (;;) {
      if (plive && !(diag & 2)) hex8_cl_produce<M>(k, X, U, AX, ED, 0, lds + pl * R::STRIDE);
      cll::lds_barrier();                   // point 0 and the lists are out; the consumers' atomics of the previous cluster are in the image
      const int nb = cb == 2 ? 0 : cb + 1;
#pragma unroll 1
      for (int q = 0; q < 8; q++) {         // one point ahead of the consumers
        if (q + 1 < 8) { if (plive && !(diag & 2)) hex8_cl_produce<M>(k, X, U, AX, ED, q + 1, lds + (((q + 1) & 1) * MAXE + pl) * R::STRIDE); }
        else if (w + G < n_wg) load_element(w + G);
        if (q == 0 && w + G < n_wg) stage_lists(w + G, nb);
        cll::lds_barrier();
      }
      cb = nb;
      w += G;
      if (w >= n_wg) break;
    }
    cll::lds_barrier();                     // the consumers' atomics of the last cluster
    return;
  }
  // ================= consumers: every global store of the workgroup ====================================================================
  double acc[NV][NV][8], fe[NV];
  int cb = 0, pb = -1;                      // list buffers of the current / previous cluster
  for (;;) {
    rd_row_zero<M, 8>(acc, fe);
    cll::lds_barrier();                     // producer: point 0 and the lists of this cluster
    const uint32_t* lb = lists + cb * L::WORDS;
    const cll::Pair pr = cll::pair_decode(lb[L::PAIR + tid]);
#pragma unroll 1
    for (int q = 0; q < 8; q++) {
      if (pb >= 0) copy_slice(pb, q, true);
      if (pr.valid && !(diag & 1)) hex8_cl_consume<M, EXP_MODE>(k, lds + ((q & 1) * MAXE + pr.le) * R::STRIDE, q, pr.li, acc, fe);
      cll::lds_barrier();
    }
    // the previous cluster's image has been copied out and zeroed during these eight rounds
    if (pr.valid && !(diag & 8)) cll::add_rows<M>(img, lrhs, cll::pair_aim(lb + L::SLOT, lb + L::NTAB, tid, pr.na), pr.na, acc, fe);
    pb = cb;
    cb = cb == 2 ? 0 : cb + 1;
    w += G;
    if (w >= n_wg) break;
  }
  cll::lds_barrier();
  for (int q = 0; q < 8; q++) copy_slice(pb, q, false);
}

template <class M>
inline size_t hex8_clp_lds_bytes(int cw, int pw, size_t max_row_doubles) {
  const size_t pbuf = cll::even((size_t)2 * cll::max_elems(pw) * Hex8Rec<M>::STRIDE);
  const size_t image = cll::even(max_row_doubles) + cll::even((size_t)M::NV * cll::max_nodes(cw));
  return sizeof(double) * (pbuf + image) + sizeof(uint32_t) * 3 * Hex8ClLists<3>::WORDS;
}

template <class M, int EXP_MODE>
static hipError_t launch_hex8_cl(const LaunchArgs& a, const typename M::K& k) {
  constexpr int CW = 3, PW = 1;
  if (a.cl.cw != CW || a.cl.pw != PW) return hipErrorInvalidValue;
  const size_t pbytes = hex8_clp_lds_bytes<M>(CW, PW, a.cl.max_row_doubles);
  if (a.cl.grid > 0 && pbytes <= 80 * 1024) {   // persistent form: two workgroups per CU must fit
    static std::atomic<uint64_t> pattr[1];  /* per instantiation and device */
    dyn_lds_once(pattr[0], (const void*)k_hex8_clp<M, EXP_MODE, CW, PW>, 80 * 1024);
    const int grid = a.cl.grid < a.cl.n_wg ? a.cl.grid : a.cl.n_wg;
    hipLaunchKernelGGL((k_hex8_clp<M, EXP_MODE, CW, PW>), dim3(grid), dim3((CW + PW) * 64), pbytes, a.stream, a.m, k, a.cl.desc, a.cl.ntab,
                       a.cl.eid, a.cl.pair, a.cl.pslot, a.u, a.aux, a.elem, a.val, a.rhs, a.cl.n_wg, cll::rhs_offset((int)a.cl.max_row_doubles), a.opt.ablate);
    return hipGetLastError();
  }
  // quadrature points per round and workgroup barrier: the model's choice (M::HEX_CL_POINTS); "prefetch" = 1 forces one
#define RDC_HEX8_CL(PPR)                                                                                                              \
  {                                                                                                                                   \
    const size_t bytes = cll::overlay_bytes((size_t)2 * PPR * cll::max_elems(PW) * Hex8Rec<M>::STRIDE, a.cl.max_row_doubles, (size_t)M::NV * cll::max_nodes(CW)); \
    static std::atomic<uint64_t> attr[1];  /* per instantiation and device */ \
    dyn_lds_once(attr[0], (const void*)k_hex8_cl<M, EXP_MODE, CW, PW, PPR>, 80 * 1024); \
    hipLaunchKernelGGL((k_hex8_cl<M, EXP_MODE, CW, PW, PPR>), dim3(a.cl.n_wg), dim3((CW + PW) * 64), bytes, a.stream, a.m, k, a.cl.desc, a.cl.ntab, \
                       a.cl.eid, a.cl.pair, a.cl.pslot, a.u, a.aux, a.elem, a.val, a.rhs, a.opt.ablate);                             \
  }
  if constexpr (M::HEX_CL_POINTS == 2) { if (a.opt.prefetch == 1) RDC_HEX8_CL(1) else RDC_HEX8_CL(2) }
  else RDC_HEX8_CL(1)
#undef RDC_HEX8_CL
  return hipGetLastError();
}

// ---- five unknowns: one equation row at a time ----------------------------------------------------------------------------
// The 5 x 5 x 8 accumulator of a pair does not fit the register file (the pair kernels evaluate such models one equation row
// at a time too, redoing the whole per-point set-up five times per pair).  Here the workgroup makes NV passes over the
// quadrature points: in pass A the producer hands out the point records again (cheap next to the consumers' work), the
// consumers accumulate row A only (NV x 8 accumulators), add it into an LDS image of equation row A of the cluster's nodes
// and the image leaves as one run of NV * len doubles per node.  The image overlays the point buffers.
template <class M, int EXP_MODE, int CW, int PW>
__global__ void __launch_bounds__((CW + PW) * 64, 2)
k_hex8_cl_rows(const MeshDev m, const typename M::K k, const HostPrepCl::Desc* __restrict__ desc, const HostPrepCl::Node* __restrict__ ntab,
               const uint32_t* __restrict__ eid, const uint32_t* __restrict__ pair, const uint32_t* __restrict__ pslot,
               const double* __restrict__ u, const double* __restrict__ aux, const double* __restrict__ elem,
               double* __restrict__ val, double* __restrict__ rhs) {
  constexpr int NV = M::NV, NA = (M::NAUX > 0 ? M::NAUX : 1), NT = (CW + PW) * 64;
  constexpr cll::Strides S = cll::strides(CW, PW);
  constexpr int MAXP = (int)S.pair, MAXE = (int)S.elem;
  using R = Hex8Rec<M>;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int w = blockIdx.x;
  const int tid = cll::role_tid<CW + PW>();
  const HostPrepCl::Desc d = desc[w];
  const int nimg = (int)d.row_doubles, nown = (int)d.nown;   // image of ONE equation row: sum of NV * len
  double* const img = lds;
  double* const lrhs = lds + cll::rhs_offset(nimg);          // one rhs entry per owned node and pass
  // a half-wave per node: equation row A of the node is NV * len consecutive doubles of the CSR array.  Not cll::copy_out: the
  // segments of a one-row image do not keep the 16-byte phase of the CSR rows (8-byte stores), and one rhs entry leaves per node
  auto copy_out = [&](int A) {
    for (int a = tid >> 5; a < nown; a += NT / 32) {
      const HostPrepCl::Node nd = ntab[(size_t)w * S.node + a];
      const int nn = NV * (int)nd.len;
      double* dst = val + (int64_t)(NV * NV) * nd.bptr + (int64_t)A * nn;
      for (int x = tid & 31; x < nn; x += 32) __builtin_nontemporal_store(img[nd.off + x], dst + x);
      if ((tid & 31) == 0) rhs[(int64_t)NV * nd.node + A] = lrhs[a];
    }
  };
  if (tid >= MAXP) {
    // ---- producer --------------------------------------------------------------------------------------------------------------
    const int pl = tid - MAXP;
    const uint32_t e = eid[(size_t)w * S.elem + pl];
    const bool plive = e != cll::IDLE;
    double X[8][3], U[8][NV], AX[8][NA];
    if (plive) cll::load_element<M>(m, e, u, aux, X, U, AX);
    const double* ED = cll::elem_data<M>(elem, e);
#pragma unroll 1
    for (int A = 0; A < NV; A++) {
      if (plive) hex8_cl_produce<M>(k, X, U, AX, ED, 0, lds + pl * R::STRIDE);
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < 8; q++) {
        if (plive && q + 1 < 8) hex8_cl_produce<M>(k, X, U, AX, ED, q + 1, lds + (((q + 1) & 1) * MAXE + pl) * R::STRIDE);
        __syncthreads();
      }
      cll::zero_image<NT>(lds, tid, nimg, nown);
      cll::lds_barrier();
      cll::lds_barrier();           // consumers: atomics of row A
      copy_out(A);
      cll::lds_barrier();           // the image has been read: the next pass may overwrite it
    }
    return;
  }
  // ---- consumers ------------------------------------------------------------------------------------------------------------------
  const cll::Pair pr = cll::pair_decode(pair[(size_t)w * S.pair + tid]);
  cll::Aim aim = {0, 0, 0, 0};
  if (pr.valid) aim = cll::pair_aim(pslot + (size_t)w * S.pslot, reinterpret_cast<const uint32_t*>(ntab + (size_t)w * S.node), tid, pr.na);
  auto pass = [&](auto tagA) {
    constexpr int A = decltype(tagA)::value;
    double acc[NV][8], fe = 0.0;
#pragma unroll
    for (int b = 0; b < NV; b++)
#pragma unroll
      for (int j = 0; j < 8; j++) acc[b][j] = 0.0;
    __syncthreads();                // producers: point 0
#pragma unroll 1
    for (int q = 0; q < 8; q++) {
      if (pr.valid) hex8_cl_consume_row<M, EXP_MODE, A>(k, lds + ((q & 1) * MAXE + pr.le) * R::STRIDE, q, pr.li, acc, fe);
      __syncthreads();
    }
    cll::zero_image<NT>(lds, tid, nimg, nown);
    cll::lds_barrier();
    if (pr.valid) {   // row A only (acc[b][j]), so not cll::add_rows
#pragma unroll
      for (int j = 0; j < 8; j++) {
#pragma unroll
        for (int b = 0; b < NV; b++)
          if (hex8_cl_block<M>(A, b))   // structurally zero blocks stay the zeros of the image
            __hip_atomic_fetch_add(img + aim.off + NV * cll::pslot_get(aim.sl0, aim.sl1, j) + b, acc[b][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __hip_atomic_fetch_add(lrhs + pr.na, fe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    cll::lds_barrier();
    copy_out(A);
    cll::lds_barrier();
  };
  pass(std::integral_constant<int, 0>{});
  pass(std::integral_constant<int, 1>{});
  pass(std::integral_constant<int, 2>{});
  if constexpr (NV > 3) pass(std::integral_constant<int, (NV > 3 ? 3 : 0)>{});
  if constexpr (NV > 4) pass(std::integral_constant<int, (NV > 4 ? 4 : 0)>{});
}

template <class M, int EXP_MODE>
static hipError_t launch_hex8_cl_rows(const LaunchArgs& a, const typename M::K& k) {
  constexpr int CW = 3, PW = 1;
  if (a.cl.cw != CW || a.cl.pw != PW) return hipErrorInvalidValue;
  // rhs: one entry per node (+ 2: what this launcher has always added for the roundings of cll::zero_doubles)
  const size_t bytes = cll::overlay_bytes((size_t)2 * cll::max_elems(PW) * Hex8Rec<M>::STRIDE, a.cl.max_row_doubles, (size_t)cll::max_nodes(CW) + 2);
  static std::atomic<uint64_t> attr[1];  /* per instantiation and device */
  dyn_lds_once(attr[0], (const void*)k_hex8_cl_rows<M, EXP_MODE, CW, PW>, 80 * 1024);
  hipLaunchKernelGGL((k_hex8_cl_rows<M, EXP_MODE, CW, PW>), dim3(a.cl.n_wg), dim3((CW + PW) * 64), bytes, a.stream, a.m, k, a.cl.desc, a.cl.ntab,
                     a.cl.eid, a.cl.pair, a.cl.pslot, a.u, a.aux, a.elem, a.val, a.rhs);
  return hipGetLastError();
}

}  // namespace rdc
#endif
