// rdc_models.h — the reaction-diffusion models as the kernel-path decision sees them (rdc_path.h): the instantiations a model has
// beside itself, which of the optional kernels it takes, and describe<M>(), which states both as a PathModel.  Host + device code of
// the models only (no HIP call): the CPU suite compiles it with g++ (tests/host_shim.cpp).
#ifndef RDC_MODELS_H
#define RDC_MODELS_H
#include <type_traits>

#include "rdc_path.h"
#include "rdc_tet4_pihna_moments.h"

namespace rdc {

// Which models run k_tet4_evc (rdc_tet4_evc.hip), measured on K(94) against k_tet4_rg5 (tools/ab.py): Ripf with all terms on 1.41 vs
// 1.79 ms (the per-element part -- two exp, sqrt, the unit gradient -- dominates); RipfReduced 0.87 vs 0.78, Hcc 0.90 vs 0.65: the
// pair kernel packs the row atomics of a wave densely, an element visit executes a row position for as few as 10 of 64 lanes
// (Pihna with all terms on, five unknowns, was tried in round 3: tet4_visit<Pihna> needs 3.9 KB of scratch per lane -- profiles/r03_ev_ab_log.md)
template <class M> struct EvcEligible { static constexpr bool value = std::is_same<M, Ripf>::value; };

// Which models (the model of the assemble call: Pihna, Ripf, Hcc, Adpm, Proteas) take the cluster kernel k_tet4_cl in mode 1 of
// rdc_tet4_cluster_mode; mode 2 forces every model.  The measurements behind MODE1 (meshes.delaunay(56),
// 1.17 M tets, against k_tet4_rowgather / k_rowgather<M, 4>): PIHNA 1.20 - 1.25 x, HCC 1.27 x, ADPM 1.90 x, PROTEAS 1.97 x faster;
// RIPF 1.00 - 1.01 x (a tie just outside the run's noise floor, and no record pack pass): every model stays in.  On a Kuhn mesh
// the established kernels are 1.1 - 2.8 x faster than this one: mode 2 is for tests and A/B
template <class M> struct Tet4ClWanted { static constexpr bool MODE1 = true; };

// The instantiations of a model beside itself (Inst): parameter-sparsity variants with smaller structural masks that are exact
// when pattern(p) holds (PIHNA with the cell transport terms off; the all-rates-zero HCC of run/Coupled/HCC and the decay-only
// ADPM of run/HCP102513, which exist for every element type and kernel).  PIHNA's sparse rows also exist in moment form
// (PihnaNoCellTransportMoments, Inst::MOMENTS).
template <class M> struct Forms {
  using Sparse = M;
  static constexpr bool TET4_ONLY = false;
  template <class P> static bool pattern(const P&) { return false; }
};
template <> struct Forms<Pihna> {
  using Sparse = PihnaNoCellTransport;
  static constexpr bool TET4_ONLY = true;
  static bool pattern(const rdc_pihna_params& p) { return Sparse::applies(p); }
};
template <> struct Forms<Ripf> {
  using Sparse = RipfReduced;
  static constexpr bool TET4_ONLY = true;
  static bool pattern(const rdc_ripf_params& p) { return Sparse::applies(p); }
};
template <> struct Forms<Hcc> {
  using Sparse = HccMassOnly;
  static constexpr bool TET4_ONLY = false;
  static bool pattern(const rdc_hcc_params& p) { return Sparse::applies(p); }
};
template <> struct Forms<Adpm> {
  using Sparse = AdpmDecayOnly;
  static constexpr bool TET4_ONLY = false;
  static bool pattern(const rdc_adpm_params& p) { return Sparse::applies(p); }
};

template <class M>
constexpr PathModel describe() {
  return {M::NV, M::NELEM > 0, M::AUX_LOCAL_NODE >= 0, std::is_same<M, Pihna>::value, EvcEligible<M>::value, Tet4ClWanted<M>::MODE1,
          Forms<M>::TET4_ONLY, Forms<M>::Sparse::NELEM > 0};
}

}  // namespace rdc
#endif
