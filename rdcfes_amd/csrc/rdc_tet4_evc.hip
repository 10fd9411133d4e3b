// rdc_tet4_evc.hip — element-visit kernel in coefficient form for three-unknown TET4 models; instantiated for Ripf (all terms
// on), the one model whose per-element part is heavy enough to win against the pair kernel (EvcEligible, rdc_models.h).  Formulation: rdc_tet4_evc.h; lists: rdc_prep_ev.cpp (the lists of k_tet4_ev).
//
// One workgroup = one CLUSTER of <= 16 owned nodes and the <= 256 elements touching it.
//   phase 0  zero the entry slice, load the lists, LDS-DMA the node records of the cluster's closure
//   phase 1  one thread per element visit: tet4_visit() -> ds_add_f64 of the entries of the rows it owns; slice layout
//            [entry of the block][slot][node] (bank = row node: the host placed the visits so that the 16 lanes of an LDS
//            pass have different row nodes)
//   phase 2  one thread per node block: its entries -> LDS image of the CSR rows of the cluster's nodes (zeros for the
//            structurally zero blocks); rhs entries straight to memory
//   phase 3  the image leaves with 16-byte non-temporal stores, one contiguous CSR segment per node
// Every CSR value is written exactly once; no global atomics, no colours.  Sums are order-dependent in the last bits.
#include "rdc_internal.h"
#include "rdc_tet4_ev.h"
#include "rdc_ev_phases.h"
#include "rdc_tet4_evc.h"

namespace rdc {

template <class M> struct EvcRec {   // node record of k_pack_nodes<M> (rdc_tet4_fast.hip): xyz | u | aux | pad
  static constexpr int RAW = 3 + M::NV + M::NAUX;
  static constexpr int N = (RAW + 1) & ~1;
};

template <class M>
struct EvcSink {
  double* p[4][4];   // LDS address of entry 0 of block (node i, node j)
  double* pr[4];     // LDS address of rhs entry 0 of node i
  __device__ __forceinline__ void ke(int a, int b, int i, int j, double v) {
    __hip_atomic_fetch_add(p[i][j] + evc_index<M>(a, b) * ev::NBP, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void fe(int a, int i, double v) {
    __hip_atomic_fetch_add(pr[i] + a * ev::MAXN, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

template <class M, int EXP_MODE, int MINW>
__global__ void __launch_bounds__(256, MINW)
k_tet4_evc(const HostPrepEv::Desc* __restrict__ desc, const uint32_t* __restrict__ nlist, const uint32_t* __restrict__ vloc,
           const uint32_t* __restrict__ vslot, const HostPrepEv::Node* __restrict__ ntab, const uint32_t* __restrict__ wg_perm,
           const typename M::K k, const double* __restrict__ rec, double* __restrict__ val, double* __restrict__ rhs,
           const int nls, const int wg_begin) {
  constexpr int BLOCK = 256, NV = M::NV, NA = (M::NAUX > 0 ? M::NAUX : 1), NP = EvcRec<M>::N / 2, NE = evc_blocks<M>();
  constexpr int NBP = ev::NBP, MAXN = ev::MAXN;
  extern __shared__ __attribute__((aligned(16))) double lds[];   // [S: NE x NBP | R: NV x MAXN | records: NP x nls x 16 B]
  __shared__ __attribute__((aligned(16))) HostPrepEv::Node snode[MAXN];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* glb_ptr;
  int w = (int)blockIdx.x + wg_begin;
  if (wg_perm) w = (int)wg_perm[w];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* const R = lds + NE * NBP;
  double* const recs = R + ((NV * MAXN + 1) & ~1);
  // phase 0: zero [S | R] (16-byte stores), list loads, LDS-DMA of the node records
  {
    double2* z = reinterpret_cast<double2*>(lds);
    for (int x = tid; x < (NE * NBP + ((NV * MAXN + 1) & ~1)) / 2; x += BLOCK) z[x] = make_double2(0.0, 0.0);
  }
  const int rounds = nls >> 6;
  uint32_t nid = 0;
  if (wv < rounds) nid = nlist[(size_t)w * nls + wv * 64 + lane];
  const uint32_t pl = vloc[(size_t)w * BLOCK + tid];
  const uint2 sl = reinterpret_cast<const uint2*>(vslot)[(size_t)w * BLOCK + tid];
  const HostPrepEv::Desc d = desc[w];
  if (tid < MAXN) snode[tid] = ntab[(size_t)w * MAXN + tid];
  if (wv < rounds) {
    const char* src = reinterpret_cast<const char*>(rec) + (size_t)nid * (NP * 16);
#pragma unroll
    for (int p = 0; p < NP; p++)
      __builtin_amdgcn_global_load_lds((glb_ptr)(src + p * 16), (lds_ptr)evl::rec_at(recs, nls, p, wv * 64), 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // phase 1: element visits
  if (pl != evl::IDLE) {
    double X[4][3], U[4][NV], AX[4][NA];
    int li[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      li[j] = evl::vloc_pos(pl, j);
      double rr[2 * NP];
#pragma unroll
      for (int p = 0; p < NP; p++) {
        const double2 v2 = evl::rec_piece(recs, nls, p, li[j]);
        rr[2 * p] = v2.x; rr[2 * p + 1] = v2.y;
      }
      X[j][0] = rr[0]; X[j][1] = rr[1]; X[j][2] = rr[2];
#pragma unroll
      for (int v = 0; v < NV; v++) U[j][v] = rr[3 + v];
#pragma unroll
      for (int v = 0; v < NA; v++) AX[j][v] = M::NAUX > 0 ? rr[(3 + NV + v) % (2 * NP)] : 0.0;
    }
    const int r = evl::vloc_rows(li, (int)d.nown);
    EvcSink<M> sink;
    evl::aim(sink, lds, R, li, r, sl);
    tet4_visit<M, EXP_MODE>(k, X, U, AX, r, sink);
  }
  __syncthreads();
  // phase 2: node block tid = evl::block(bn, bs)
  double e[NE];
  const int bn = evl::block_node(tid), bs = evl::block_slot(tid);
  const bool has = bn < (int)d.nown && bs < (int)snode[bn < (int)d.nown ? bn : 0].len;
  if (has) {
#pragma unroll
    for (int m = 0; m < NE; m++) e[m] = lds[m * NBP + tid];
  }
  if (tid < (int)d.nown * NV) {   // rhs: R[a][node] -> rhs[node * NV + a]
    const int n = tid / NV, a = tid - n * NV;
    rhs[(size_t)snode[n].node * NV + a] = R[a * MAXN + n];
  }
  __syncthreads();   // every entry has been read: the image may overwrite the slice
  if (has) {
    const int len = (int)snode[bn].len;
    double* dst = lds + snode[bn].obase + evl::seg_entry(NV, len, 0, bs, 0);
#pragma unroll
    for (int a = 0; a < NV; a++)
#pragma unroll
      for (int b = 0; b < NV; b++) dst[evl::seg_entry(NV, len, a, 0, b)] = evc_block<M>(a, b) ? e[evc_index<M>(a, b) % NE] : 0.0;
  }
  __syncthreads();
  // phase 3: one contiguous CSR segment per node; the image has the 16-byte phase of its segment in memory
  {
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    if constexpr (MINW == 2) {   // nodes wv, wv + 4, wv + 8, wv + 12: two at a time
      HostPrepEv::Node nd[4];
      evl::wave_nodes(snode, wvu, nd);
      const HostPrepEv::Node nd01[2] = {nd[0], nd[1]}, nd23[2] = {nd[2], nd[3]};
      const bool on01[2] = {wvu < (int)d.nown, wvu + 4 < (int)d.nown}, on23[2] = {wvu + 8 < (int)d.nown, wvu + 12 < (int)d.nown};
      if (on01[0]) evl::store_segments<NV * NV, 2>(lds, val, nd01, on01, lane);
      if (on23[0]) evl::store_segments<NV * NV, 2>(lds, val, nd23, on23, lane);
    } else {                     // three workgroups per CU: the visit spills, and what a second segment keeps in registers would add to that
#pragma unroll 1
      for (int n = wvu; n < (int)d.nown; n += 4) {
        HostPrepEv::Node nd1[1];
        evl::wave_nodes(snode, n, nd1);
        const bool on1[1] = {true};
        evl::store_segments<NV * NV, 1>(lds, val, nd1, on1, lane);
      }
    }
  }
}

// the node records have been packed by the caller (launch_fast_impl, rdc_tet4_fast.hip)
template <class M>
hipError_t launch_tet4_evc(const LaunchArgs& a, const typename M::K& k) {
  const EvDev& E = a.ev;
  const int wg_count = E.wg_count < 0 ? E.n_wg - E.wg_begin : E.wg_count;
  if (wg_count <= 0) return hipSuccess;
  constexpr int NE = evc_blocks<M>(), NP = EvcRec<M>::N / 2;
  const size_t acc = (size_t)NE * ev::NBP + ((M::NV * ev::MAXN + 1) & ~1) + (size_t)NP * E.nls * 2;
  const size_t lds_bytes = sizeof(double) * (acc > E.max_out_doubles ? acc : E.max_out_doubles);
#define RDC_EVC(MODE, MINW)                                                                                                \
  hipLaunchKernelGGL((k_tet4_evc<M, MODE, MINW>), dim3(wg_count), dim3(256), lds_bytes, a.stream, E.desc, E.nlist, E.vloc, \
                     E.vslot, E.ntab, E.wg_perm, k, a.packed, a.val, a.rhs, E.nls, E.wg_begin)
  if (a.opt.evc_occupancy == 3) { if (a.exp_mode == M::FAST_EXP_MODE) RDC_EVC(M::FAST_EXP_MODE, 3); else RDC_EVC(0, 3); }
  else { if (a.exp_mode == M::FAST_EXP_MODE) RDC_EVC(M::FAST_EXP_MODE, 2); else RDC_EVC(0, 2); }
#undef RDC_EVC
  return hipGetLastError();
}

template hipError_t launch_tet4_evc<Ripf>(const LaunchArgs&, const Ripf::K&);

}  // namespace rdc
