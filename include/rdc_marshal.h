// rdc_marshal.h — what a host binding does between a string-keyed parameter store and the C-ABI (rdc_assembly.h), stated
// once: which reference key fills which struct field, the material table and the side list of the solid system, the
// error path, and the pipelined hand-back of the assembled rows.  integration/libmesh_adapter.C includes it with
// libMesh::Parameters, rdcfes_amd/host/rdc_host.h with its own; tests/test_host_marshal.py pins the tables to params.py.
//
// Header-only, C++17, the C-ABI and the standard library only.  A parameter store P offers exactly
//     template <class T> const T& get(const std::string&) const;             (throws, or aborts, on a missing key)
//     template <class T> bool have_parameter(const std::string&) const;
// Reals are read as double (libMesh's default Real, which the reference is built with), "RT_dose/total/max" as int.
#ifndef RDC_MARSHAL_H
#define RDC_MARSHAL_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "rdc_assembly.h"

namespace rdc {
namespace marshal {

// the one error path: a failing C-ABI status becomes a std::runtime_error with the call's name and rdc_last_error
inline void check(const rdc_ctx* c, int rc, const char* what) {
  if (rc != RDC_OK) throw std::runtime_error(std::string(what) + ": " + rdc_last_error(c));
}

// ---- key tables: (reference key, byte offset of the field, int or real), in the order the reference reads them ----
struct Key { std::string key; size_t offset; bool is_int; };
using KeyTable = std::vector<Key>;
template <class S> const KeyTable& keys();

#define RDC_KEY_TABLE(STRUCT, ...) \
  template <> inline const KeyTable& keys<STRUCT>() { using S = STRUCT; static const KeyTable t = __VA_ARGS__; return t; }
#define RDC_K(key, field) {key, offsetof(S, field), false}

RDC_KEY_TABLE(rdc_pihna_params, {   // src/pihna.C:358-381
    RDC_K("time_step", time_step), RDC_K("cells_min_capacity", cells_min_capacity), RDC_K("cells_max_capacity", cells_max_capacity),
    RDC_K("cytokines_max_capacity", cytokines_max_capacity), RDC_K("cells_max_capacity/exponent", cells_max_capacity_exponent),
    RDC_K("necrosis/c", necrosis_c), RDC_K("necrosis/h", necrosis_h), RDC_K("necrosis/v", necrosis_v), RDC_K("diffuse/c", diffuse_c), RDC_K("taxis/c", taxis_c),
    RDC_K("diffuse/h", diffuse_h), RDC_K("taxis/h", taxis_h), RDC_K("produce/c", produce_c), RDC_K("switch/c/to/h", switch_c2h), RDC_K("switch/h/to/c", switch_h2c),
    RDC_K("switch/h/to/n", switch_h2n), RDC_K("diffuse/v", diffuse_v), RDC_K("taxis/v", taxis_v), RDC_K("produce/v", produce_v),
    RDC_K("secrete/a/from/c", secrete_a_c), RDC_K("secrete/a/from/h", secrete_a_h), RDC_K("uptake/a/from/v", uptake_a_v), RDC_K("decay/a", decay_a)})

RDC_KEY_TABLE(rdc_ripf_params, {   // src/ripf.C:377-408
    RDC_K("time_step", time_step), RDC_K("volume_fraction/stroma", VolFr_stroma), RDC_K("volume_fraction/parenchyma", VolFr_parenchyma),
    RDC_K("volume_fraction/exponent", VolFr_exponent), RDC_K("volume_fraction/min_vacant", VolFr_min_vacant), RDC_K("volume_fraction/max_vacant", VolFr_max_vacant),
    RDC_K("HU/phi/cc/build", phi_cc_B), RDC_K("HU/phi/cc/decay", phi_cc_D), RDC_K("HU/phi/cc/rate", phi_cc), RDC_K("HU/phi/fb/build", phi_fb_B),
    RDC_K("HU/phi/fb/decay", phi_fb_D), RDC_K("HU/phi/fb/rate", phi_fb), RDC_K("HU/phi/tolerance", phi_tol), RDC_K("cc/kappa", kappa), RDC_K("cc/kappa/RT/c", kappa_RT_c),
    RDC_K("cc/delta", delta), RDC_K("cc/delta/RT/a", delta_RT_a), RDC_K("cc/delta/RT/b", delta_RT_b), RDC_K("fb/lambda", lambda), RDC_K("fb/lambda/RT/r", lambda_RT_r),
    RDC_K("fb/lambda/HU/r", lambda_HU_r), RDC_K("fb/omicro", omicro), RDC_K("fb/omicro/RT/r", omicro_RT_r), RDC_K("fb/omicro/fb/b", omicro_fb_b), RDC_K("fb/omega", omega),
    RDC_K("fb/diffusion", diffusion), RDC_K("fb/haptotaxis", haptotaxis), RDC_K("fb/radiotaxis", radiotaxis),
    {"RT_dose/total/max", offsetof(S, RT_dose_total_max), true}})

RDC_KEY_TABLE(rdc_hcc_params, {   // src/coupled_hcc.C:450-461
    RDC_K("time_step", time_step), RDC_K("cells/min_capacity", cells_min_capacity), RDC_K("cells/max_capacity", cells_max_capacity),
    RDC_K("cells/max_capacity/exponent", cells_max_capacity_exponent), RDC_K("produce/l", produce_l), RDC_K("diffuse/c", diffuse_c), RDC_K("mechano/c", mechano_c),
    RDC_K("produce/c", produce_c), RDC_K("necrosis/l", necrosis_l), RDC_K("necrosis/c", necrosis_c), RDC_K("necrosis/pressure", necrosis_pressure)})

// src/adpm.C:367-413: a coefficient with its pulse / sigmoid pair or its trapezoid quadruple is one array of the struct,
// {"<key>", "<key>/pulse/0", "<key>/pulse/1"}.  `time` is system.time, not a key; the angles are stored in radians (src/adpm.C:193).
RDC_KEY_TABLE(rdc_adpm_params, [] {
  KeyTable k = {RDC_K("time_step", time_step), RDC_K("decay/PrP/time_exponent", decay_PrP_time_exponent)};
  auto shaped = [&k](const std::string& key, size_t offset, const char* shape, int n) {
    k.push_back({key, offset, false});
    for (int i = 0; i < n; i++) k.push_back({key + shape + std::to_string(i), offset + (size_t)(i + 1) * sizeof(double), false});
  };
  shaped("decay/PrP", offsetof(S, decay_PrP), "/pulse/", 2);
  shaped("transform/A_b", offsetof(S, transform_A_b), "/trapezoid/", 4);
  shaped("transform/Tau", offsetof(S, transform_Tau), "/trapezoid/", 4);
  shaped("diffuse/A_b", offsetof(S, diffuse_A_b), "/pulse/", 2);
  shaped("taxis_1/A_b", offsetof(S, taxis1_A_b), "/pulse/", 2);
  shaped("taxis_2/A_b", offsetof(S, taxis2_A_b), "/pulse/", 2);
  shaped("produce/A_b", offsetof(S, produce_A_b), "/sigmoid/", 2);
  shaped("decay/A_b", offsetof(S, decay_A_b), "/pulse/", 2);
  shaped("diffuse/Tau", offsetof(S, diffuse_Tau), "/pulse/", 2);
  shaped("taxis_1/Tau", offsetof(S, taxis1_Tau), "/pulse/", 2);
  shaped("taxis_2/Tau", offsetof(S, taxis2_Tau), "/pulse/", 2);
  shaped("produce/Tau", offsetof(S, produce_Tau), "/sigmoid/", 2);
  shaped("decay/Tau", offsetof(S, decay_Tau), "/pulse/", 2);
  k.push_back(RDC_K("taxis/A_b/angle", taxis_A_b_angle));
  k.push_back(RDC_K("taxis/Tau/angle", taxis_Tau_angle));
  return k;
}())

RDC_KEY_TABLE(rdc_proteas_params, {   // src/proteas.C:376-409
    RDC_K("time_step", time_step), RDC_K("cells/total_capacity", cells_total_capacity), RDC_K("radiotherapy/max_dosage", RT_max_dosage),
    RDC_K("host/proliferation", host_proliferation), RDC_K("host/vsc_threshold", host_vsc_threshold), RDC_K("host/RT_death_rate", host_RT_death_rate),
    RDC_K("host/RT_exp_a", host_RT_exp_a), RDC_K("host/RT_exp_b", host_RT_exp_b), RDC_K("host/necrosis_rate", host_necrosis_rate),
    RDC_K("tumour/diffusion", tumour_diffusion), RDC_K("tumour/diffusion_host", tumour_diffusion_host), RDC_K("tumour/proliferation", tumour_proliferation),
    RDC_K("tumour/vsc_threshold", tumour_vsc_threshold), RDC_K("tumour/RT_death_rate", tumour_RT_death_rate), RDC_K("tumour/RT_exp_a", tumour_RT_exp_a),
    RDC_K("tumour/RT_exp_b", tumour_RT_exp_b), RDC_K("tumour/necrosis_rate", tumour_necrosis_rate), RDC_K("necrosis/clearance", necrosis_clearance),
    RDC_K("necrosis/slope", necrosis_slope), RDC_K("necrosis/vsc_threshold", necrosis_vsc_threshold), RDC_K("vascular/proliferation", vascular_proliferation),
    RDC_K("vascular/necrosis_rate", vascular_necrosis_rate), RDC_K("oedema/diffusion", oedema_diffusion), RDC_K("oedema/proliferation", oedema_proliferation),
    RDC_K("oedema/vsc_threshold", oedema_vsc_threshold), RDC_K("oedema/RT_coeff", oedema_RT_coeff), RDC_K("oedema/RT_exp", oedema_RT_exp),
    RDC_K("oedema/reabsorption_rate", oedema_reabsorption_rate)})

RDC_KEY_TABLE(rdc_pihna_ranges, {   // save_solution, src/pihna.C:853-861
    RDC_K("range/active_tumor/min", active_tumor_min), RDC_K("range/active_tumor/max", active_tumor_max), RDC_K("range/necrotic/min", necrotic_min),
    RDC_K("range/necrotic/max", necrotic_max), RDC_K("range/vascularity/min", vascularity_min), RDC_K("range/vascularity/max", vascularity_max),
    RDC_K("range/total_cell/min", total_cell_min), RDC_K("range/total_cell/max", total_cell_max), RDC_K("cells_max_capacity", cells_max_capacity)})

RDC_KEY_TABLE(rdc_ripf_ranges, {   // save_solution, src/ripf.C:790-795
    RDC_K("range_cc/HU/min", cc_HU_min), RDC_K("range_cc/HU/max", cc_HU_max), RDC_K("range_cc/min", cc_min),
    RDC_K("range_fb/HU/min", fb_HU_min), RDC_K("range_fb/HU/max", fb_HU_max), RDC_K("range_fb/min", fb_min)})

#undef RDC_K
#undef RDC_KEY_TABLE

// the one reader: every byte of the struct zero (padding included), then every key of its table; a missing key is what P::get makes of it
template <class S, class P> S read(const P& params) {
  S s;
  std::memset(&s, 0, sizeof s);
  for (const Key& k : keys<S>()) {
    char* field = reinterpret_cast<char*>(&s) + k.offset;
    if (k.is_int) { const int32_t v = params.template get<int>(k.key); std::memcpy(field, &v, sizeof v); }
    else { const double v = params.template get<double>(k.key); std::memcpy(field, &v, sizeof v); }
  }
  return s;
}
template <class P> rdc_adpm_params read_adpm(const P& params, double time) {
  rdc_adpm_params s = read<rdc_adpm_params>(params);
  s.time = time;
  return s;
}

// ---- the solid system's pieces that are not flat (src/solid_system.C:181-190, :234, :291-306) ----
template <class P> rdc_solid_params solid_params(const P& params) {
  return {params.template get<double>("pseudo_time"), params.template get<double>("BCs/displacement_penalty"),
          params.template get<bool>("solver/assembly_use_symmetry") ? 1 : 0, /*_pad*/ 0};
}

template <class P> rdc_solid_material solid_material(const P& params, int subdomain_id) {
  const std::string k = "material/" + std::to_string(subdomain_id) + "/Hyperelastic/";
  auto real = [&](const std::string& name) { return params.template get<double>(k + name); };
  return {real("Young"), real("Poisson"), real("FibreStiffness"),
          {real("VolumetricStretchRatio/rate_0"), real("VolumetricStretchRatio/rate_1"), real("VolumetricStretchRatio/rate_2")}};
}

// one table entry per subdomain id present, in the order the elements meet them; subdomain_of(e) = elem->subdomain_id()
struct MaterialTable { std::vector<int32_t> elem_material; std::vector<rdc_solid_material> table; };
template <class P, class SubdomainOf> MaterialTable material_table(const P& params, int64_t n_elem, SubdomainOf&& subdomain_of) {
  MaterialTable t;
  std::map<int, int32_t> index;
  for (int64_t e = 0; e < n_elem; e++) {
    const int id = (int)subdomain_of(e);
    auto it = index.find(id);
    if (it == index.end()) {
      it = index.emplace(id, (int32_t)t.table.size()).first;
      t.table.push_back(solid_material(params, id));
    }
    t.elem_material.push_back(it->second);
  }
  return t;
}

// src/utils.h:268-288: the integers of a blank-separated string ("BCs", "materials", "loading_time_points")
inline std::set<int> export_integers(const std::string& s) {
  std::set<int> numbers;
  std::stringstream ss(s);
  for (std::string tmp; ss >> tmp;) {
    int n;
    if (std::stringstream(tmp) >> n) numbers.insert(n);
  }
  return numbers;
}

// The boundary sides whose id is in "BCs", by ascending id, each with "BC/<id>/displacement" (a NaN component is not
// constrained).  sides_of(id, emit) calls emit(elem, side) for every side with that id, in the binding's element order.
// Point is the store's point type (libMesh::Point); only operator()(int) is used.
struct SideList { std::vector<int64_t> elem; std::vector<int32_t> side; std::vector<double> displacement; };
template <class Point, class P, class SidesOf> SideList side_list(const P& params, SidesOf&& sides_of) {
  SideList l;
  for (int bc : export_integers(params.template get<std::string>("BCs"))) {
    const Point& u = params.template get<Point>("BC/" + std::to_string(bc) + "/displacement");
    sides_of(bc, [&](int64_t elem, int32_t side) {
      l.elem.push_back(elem);
      l.side.push_back(side);
      for (int d = 0; d < 3; d++) l.displacement.push_back(u(d));
    });
  }
  return l;
}

// ---- hand-back of the assembled owned rows, pipelined ----
// Which arrays are registered with the HIP runtime (rdc_host_pin) for a context.  Kept by the caller next to the context:
// pinned on the first hand-back, pinned again only when a data pointer or a size has changed (a vector that reallocated),
// unpinned by release(), which the owner calls before rdc_ctx_destroy.
struct PinState {
  void* ptr[2] = {nullptr, nullptr};
  size_t bytes[2] = {0, 0};
  void ensure(rdc_ctx* c, double* val, size_t n_val, double* rhs, size_t n_rhs) {
    void* const want[2] = {val, rhs};
    const size_t size[2] = {n_val * sizeof(double), n_rhs * sizeof(double)};
    if (want[0] == ptr[0] && want[1] == ptr[1] && size[0] == bytes[0] && size[1] == bytes[1]) return;
    (void)release(c);   // the old arrays may be gone already: their registration is dropped as far as the runtime still can
    for (int i = 0; i < 2; i++) {
      check(c, rdc_host_pin(c, want[i], size[i]), "rdc_host_pin");
      ptr[i] = want[i];
      bytes[i] = size[i];
    }
  }
  // never throws (owners call it from destructors): the first failing status, for a caller that wants to check() it
  int release(rdc_ctx* c) noexcept {
    int rc = RDC_OK;
    for (int i = 0; i < 2; i++) {
      const int r = ptr[i] ? rdc_host_unpin(c, ptr[i]) : RDC_OK;
      if (rc == RDC_OK) rc = r;
      ptr[i] = nullptr;
      bytes[i] = 0;
    }
    return rc;
  }
};

// The owned node range [0, n_nodes) is cut into n_chunks ranges (empty ones included); rdc_csr_download_rows_async copies
// the rows of a range into their positions in the full-size val / rhs on the context's copy stream -- behind the work
// enqueued so far, independent of later work --; chunk k + 1 is enqueued before chunk k is waited for, so two tickets
// alternate; consume(n0, n1) runs when the rows of nodes [n0, n1) are in host memory, while the next chunk travels.
template <class Consume>
void hand_back_chunked(rdc_ctx* c, int64_t n_nodes, int n_chunks, double* val, size_t n_val, double* rhs, size_t n_rhs,
                       PinState& pins, Consume&& consume) {
  if (n_chunks < 1) n_chunks = 1;
  pins.ensure(c, val, n_val, rhs, n_rhs);
  auto bound = [&](int k) { return n_nodes * k / n_chunks; };
  int ticket[2] = {-1, -1};
  check(c, rdc_csr_download_rows_async(c, bound(0), bound(1), val, rhs, &ticket[0]), "rdc_csr_download_rows_async");
  for (int k = 0; k < n_chunks; k++) {
    if (k + 1 < n_chunks)
      check(c, rdc_csr_download_rows_async(c, bound(k + 1), bound(k + 2), val, rhs, &ticket[(k + 1) & 1]), "rdc_csr_download_rows_async");
    check(c, rdc_ticket_wait(c, ticket[k & 1]), "rdc_ticket_wait");
    consume(bound(k), bound(k + 1));
  }
}

}  // namespace marshal
}  // namespace rdc
#endif
