// rdc_launch.h — launchers of the generic kernels and the HEX8 cluster kernels: the path of the plan, per (element type, exponent mode).
// Included by one translation unit per model so the models compile in parallel.
#ifndef RDC_LAUNCH_H
#define RDC_LAUNCH_H
#include "rdc_internal.h"
#include "rdc_hex8_cl_kernel.h"

namespace rdc {

template <class M, int NEN, int EXP_MODE>
static hipError_t launch_rd_impl(const LaunchArgs& a, const typename M::K& k) {
  if (a.ev_start) (void)hipEventRecord(a.ev_start, a.stream);
  constexpr int BLOCK = 256;
  switch (a.plan.path) {
    case Path::HEX8_CL:        // producer / consumer cluster kernel (rdc_hex8_cl.h) on the lists the context built
      if constexpr (NEN == 8 && M::NV == 3) return launch_hex8_cl<M, EXP_MODE>(a, k);
      break;
    case Path::HEX8_CL_ROWS:   // five unknowns: the cluster kernel one equation row at a time
      if constexpr (NEN == 8 && M::NV == 5) return launch_hex8_cl_rows<M, EXP_MODE>(a, k);
      break;
    case Path::GENERIC_ROWGATHER:
      if (a.n_wg <= 0) return hipGetLastError();
      if constexpr (NEN == 8) {
        // node-staged form when the workgroup's row slice and node table fit 80 KB of LDS (two workgroups per CU)
        constexpr int REC = 3 + M::NV + (M::NAUX > 0 ? M::NAUX : 0);
        const size_t tab_off = (a.lds_bytes / sizeof(double) + 3) & ~(size_t)1;  // + slice phase shift, rounded to 16 bytes
        const size_t staged_bytes = sizeof(double) * (tab_off + (size_t)a.hx_max_nodes * REC);
        // "staged": 1 = where the model profits (M::HEX_STAGED), 2 = always, 0 = never
        if ((a.opt.staged == 2 || (a.opt.staged == 1 && M::HEX_STAGED)) && a.hx_ploc && staged_bytes <= 80 * 1024) {
          static std::atomic<uint64_t> attr_set[1];  /* per instantiation and device */
          dyn_lds_once(attr_set[0], (const void*)k_rowgather_staged<M, NEN, EXP_MODE, BLOCK>, 80 * 1024);
          hipLaunchKernelGGL((k_rowgather_staged<M, NEN, EXP_MODE, BLOCK>), dim3(a.n_wg), dim3(BLOCK), staged_bytes, a.stream,
                             a.m, k, a.u, a.aux, a.elem, a.hx_nl_ptr, a.hx_nlist, a.hx_ploc, (int)tab_off, a.val, a.rhs);
          return hipGetLastError();
        }
      }
      hipLaunchKernelGGL((k_rowgather<M, NEN, EXP_MODE, BLOCK>), dim3(a.n_wg), dim3(BLOCK), a.lds_bytes + 16,
                         a.stream, a.m, k, a.u, a.aux, a.elem, a.val, a.rhs);
      return hipGetLastError();
    case Path::GENERIC_COLOURED:
      // one launch per colour, stream order is the only synchronisation needed
      for (int c = 0; c < a.n_colours; c++) {
        const int64_t first = a.colour_ptr[c], count = a.colour_ptr[c + 1] - first;
        if (count <= 0) continue;
        const int64_t grid = (count + BLOCK - 1) / BLOCK;
        hipLaunchKernelGGL((k_coloured<M, NEN, EXP_MODE>), dim3((unsigned)grid), dim3(BLOCK), 0, a.stream, a.m, k,
                           first, count, a.u, a.aux, a.elem, a.val, a.rhs);
      }
      return hipGetLastError();
    default: break;
  }
  return hipErrorInvalidValue;   // a path this instantiation or element type does not have
}

template <class M>
hipError_t launch_rd(const LaunchArgs& a, const typename M::K& k) {
  if (a.nen == 4) {
    if (a.exp_mode == M::FAST_EXP_MODE) return launch_rd_impl<M, 4, M::FAST_EXP_MODE>(a, k);
    return launch_rd_impl<M, 4, 0>(a, k);
  }
  if (a.exp_mode == M::FAST_EXP_MODE) return launch_rd_impl<M, 8, M::FAST_EXP_MODE>(a, k);
  return launch_rd_impl<M, 8, 0>(a, k);
}

}  // namespace rdc
#endif
