// rdc_tet4_cl.hip — k_tet4_cl: the TET4 cluster kernel (rdc_tet4_cl.h) and its launcher.
#include "rdc_internal.h"
#include "rdc_cl_phases.h"
#include "rdc_tet4_cl.h"
#include "rdc_tet4_pihna_moments.h"

namespace rdc {

// A 256-thread workgroup per cluster; three phases separated by LDS-only barriers.  The lists are indexed by blockIdx.x (a
// two-part call passes the views of its sub-range).  rec_off: doubles between the image and the element records
template <class M, int EXP_MODE>
__global__ void __launch_bounds__(256, 2)
k_tet4_cl(const MeshDev m, const typename M::K k, const HostPrepCl::Desc* __restrict__ desc, const HostPrepCl::Node* __restrict__ ntab,
          const uint32_t* __restrict__ eid, const uint32_t* __restrict__ pair, const uint32_t* __restrict__ pslot,
          const double* __restrict__ u, const double* __restrict__ aux, const double* __restrict__ elem,
          double* __restrict__ val, double* __restrict__ rhs, const int rec_off) {
  constexpr int NV = M::NV, NT = 256;
  constexpr cll::Strides S = cll::strides(cll::tet4_limits(NV), 4);
  constexpr int MAXE = (int)S.elem;
  static_assert(S.pair == NT && S.pslot == NT, "a lane per pair, one slot word per pair");
  static_assert(S.node <= 2 * (NT / 32), "copy-out: a half-wave per node, at most two rounds");
  using R = Tet4ClRec<M>;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int w = blockIdx.x, tid = threadIdx.x;
  const HostPrepCl::Desc d = desc[w];
  const int nimg = (int)d.row_doubles, nown = d.nown;
  double* const img = lds;
  double* const lrhs = img + cll::rhs_offset(nimg);
  double* const recs = lds + rec_off;
  // ---- stage: the element records; the image is zeroed while the gathers are in flight --------------------------------------
  const uint32_t pw = pair[(size_t)w * S.pair + tid];
  const uint32_t e = tid < MAXE ? eid[(size_t)w * S.elem + tid] : cll::IDLE;
  double r[R::N];
  if (e != cll::IDLE) tet4_cl_gather<M>(m.conn, e, m.xyz, u, aux, r);
  cll::zero_image<NT>(img, tid, nimg, NV * nown);
  if (e != cll::IDLE) {
    double* dst = recs + tid * R::STRIDE;
#pragma unroll
    for (int x = 0; x < R::N; x++) dst[x] = r[x];
  }
  const cll::Pair pr = cll::pair_decode(pw);
  uint32_t slots = 0, nw1 = 0;
  const double* ED = nullptr;
  if (pr.valid) {
    slots = pslot[(size_t)w * S.pslot + tid];
    nw1 = reinterpret_cast<const uint32_t*>(ntab + (size_t)w * S.node)[cll::NODE_WORDS * pr.na + 1];
    if (M::NELEM > 0) ED = elem + (size_t)eid[(size_t)w * S.elem + pr.le] * M::NELEM;
  }
  cll::lds_barrier();
  // ---- rows: one pair per lane -----------------------------------------------------------------------------------------
  if (pr.valid)
    tet4_cl_pair<M, EXP_MODE>(k, recs + pr.le * R::STRIDE, pr.li, slots, img + cll::node_word_off(nw1), cll::node_word_len(nw1),
                              lrhs + NV * pr.na, ED);
  cll::lds_barrier();
  // ---- copy-out ----------------------------------------------------------------------------------------------------------
  cll::copy_out<NV, NT>(ntab + (size_t)w * S.node, nown, tid, img, lrhs, val, rhs, false);
}

template <class M, int EXP_MODE>
static hipError_t launch_tet4_cl_impl(const LaunchArgs& a, const typename M::K& k) {
  if (a.ev_start) (void)hipEventRecord(a.ev_start, a.stream);
  if (a.cl.n_wg <= 0) return hipSuccess;
  const size_t bytes = tet4_cl_lds_bytes<M>(a.cl.max_row_doubles);
  static std::atomic<uint64_t> attr[1];  /* per instantiation and device */
  dyn_lds_once(attr[0], (const void*)k_tet4_cl<M, EXP_MODE>, 160 * 1024);
  hipLaunchKernelGGL((k_tet4_cl<M, EXP_MODE>), dim3(a.cl.n_wg), dim3(256), bytes, a.stream, a.m, k, a.cl.desc, a.cl.ntab, a.cl.eid,
                     a.cl.pair, a.cl.pslot, a.u, a.aux, a.elem, a.val, a.rhs, (int)tet4_cl_rec_offset<M>(a.cl.max_row_doubles));
  return hipGetLastError();
}

template <class M>
hipError_t launch_tet4_cl(const LaunchArgs& a, const typename M::K& k) {
  if (a.exp_mode == M::FAST_EXP_MODE) return launch_tet4_cl_impl<M, M::FAST_EXP_MODE>(a, k);
  return launch_tet4_cl_impl<M, 0>(a, k);
}

template hipError_t launch_tet4_cl<Pihna>(const LaunchArgs&, const Pihna::K&);
template hipError_t launch_tet4_cl<PihnaNoCellTransport>(const LaunchArgs&, const PihnaNoCellTransport::K&);
template hipError_t launch_tet4_cl<PihnaNoCellTransportMoments>(const LaunchArgs&, const PihnaNoCellTransportMoments::K&);
template hipError_t launch_tet4_cl<Ripf>(const LaunchArgs&, const Ripf::K&);
template hipError_t launch_tet4_cl<RipfReduced>(const LaunchArgs&, const RipfReduced::K&);
template hipError_t launch_tet4_cl<Hcc>(const LaunchArgs&, const Hcc::K&);
template hipError_t launch_tet4_cl<HccMassOnly>(const LaunchArgs&, const HccMassOnly::K&);
template hipError_t launch_tet4_cl<Adpm>(const LaunchArgs&, const Adpm::K&);
template hipError_t launch_tet4_cl<AdpmDecayOnly>(const LaunchArgs&, const AdpmDecayOnly::K&);
template hipError_t launch_tet4_cl<Proteas>(const LaunchArgs&, const Proteas::K&);

}  // namespace rdc
